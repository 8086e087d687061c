// shutter.hpp — the temporal box filter behind the shutter entry points (include/maray_hip.h, "shutter"): n frames of
// one context, rendered one after the other into scratch in HBM, reduced to their integer mean by maray_shutter_reduce
// (shutter.hip).  Builds no program's kernels: not part of a code key.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "expr.hpp"
#include "maray_hip.h"

namespace maray {

constexpr uint32_t SHUTTER_GROUP = 8;       // frames one pass of the reduce reads

// One pass: the byte-wise sum of n_frames frames (+ acc_in), kept as 16-bit partial sums (acc_out) or rounded, shifted
// and written as bytes (dst).  Every frame pointer and dst are congruent modulo 16; acc_in / acc_out are congruent with
// them counted in elements (their byte address modulo 32 is twice dst's modulo 16).  acc_in == acc_out is allowed.
struct ShutterArgs {
    const unsigned char *frames[SHUTTER_GROUP];
    const unsigned short *acc_in;       // null: the sum starts at 0
    unsigned short *acc_out;            // null: this pass writes dst
    unsigned char *dst;
    size_t bytes;
    uint32_t n_frames;                  // 1 .. SHUTTER_GROUP
    uint32_t round, shift;              // dst byte = (sum + round) >> shift
};

void shutter_reduce(const ShutterArgs &a, hipStream_t st);      // enqueues one pass; throws Error

// The same pass in linear light (include/maray_hip.h, "transfer"; maray_shutter_reduce_lin, linear.hip): every frame byte is
// decoded to 16 bits, the partial sums are 32-bit (64 * 65535 needs 22 bits) in plain element order, and the last pass rounds,
// shifts and encodes.  Frames and dst congruent modulo 16; acc_in / acc_out congruent with them counted in elements (their
// byte address modulo 64 is four times dst's modulo 16).
struct ShutterLinArgs {
    const unsigned char *frames[SHUTTER_GROUP];
    const uint32_t *acc_in;
    uint32_t *acc_out;
    unsigned char *dst;
    size_t bytes;
    uint32_t n_frames;
    uint32_t round, shift;              // dst byte = E((sum + round) >> shift)
};
void shutter_reduce_lin(const ShutterLinArgs &a, hipStream_t st);
uint32_t shutter_reduce_blocks(size_t bytes);                   // its grid (blocks of 256 lanes, 16 bytes per lane and step)

inline bool shutter_frames_ok(uint32_t n) { return n && n <= 64 && (n & (n - 1)) == 0; }
inline uint32_t shutter_log2(uint32_t n) { uint32_t s = 0; while ((1u << s) < n) s++; return s; }

// The context's shutter scratch: min(n, 8) frame slots of F = round_up(bytes + 16, 256) bytes each and, for n > 8, one
// plane of 16-bit partial sums of 2 F bytes: min(n, 8) F + (n > 8 ? 2 F : 0) bytes for a raster of `bytes` bytes (`lin`, a
// MARAY_TRANSFER_SRGB context: 32-bit partial sums, 4 F).  Grows to the largest call, is freed with the context, and is
// ordered by the stream like the context's other tables.
struct ShutterScratch {
    unsigned char *base = nullptr;
    size_t cap = 0;
    static size_t slot_bytes(size_t bytes) { return (bytes + 16 + 255) / 256 * 256; }
    static size_t need(size_t bytes, uint32_t n, bool lin = false) { return (std::min(n, SHUTTER_GROUP) + (n > SHUTTER_GROUP ? (lin ? 4u : 2u) : 0u)) * slot_bytes(bytes); }
    void ensure(size_t bytes, uint32_t n, bool lin = false);      // throws Error
    void release();
};

// n frames (n in 2 .. 64, a power of two) into dst: for each, set(row) and render(frame) -- the back-end's set_params and
// its ordinary launch on `st` -- and after every group of up to 8 one pass of the reduce on the same stream.  transfer =
// MARAY_TRANSFER_SRGB: the frames are rendered the same way and reduced in linear light.
template <typename Set, typename Render>
void shutter_render(ShutterScratch &S, const double *values, uint32_t n, uint32_t n_params, size_t bytes, unsigned char *dst, hipStream_t st,
                    Set set, Render render, uint32_t transfer = MARAY_TRANSFER_NONE)
{
    const bool lin = transfer == MARAY_TRANSFER_SRGB;
    S.ensure(bytes, n, lin);
    const size_t F = ShutterScratch::slot_bytes(bytes), mis = (size_t)((uintptr_t)dst & 15);
    if (lin) {
        uint32_t *acc = n > SHUTTER_GROUP ? (uint32_t *)(S.base + SHUTTER_GROUP * F) + mis : nullptr;
        for (uint32_t g0 = 0; g0 < n; g0 += SHUTTER_GROUP) {
            ShutterLinArgs a{};
            a.n_frames = std::min(SHUTTER_GROUP, n - g0);
            for (uint32_t k = 0; k < a.n_frames; k++) {
                unsigned char *frame = S.base + k * F + mis;
                set(values + (size_t)(g0 + k) * n_params);
                render(frame);
                a.frames[k] = frame;
            }
            const bool last = g0 + SHUTTER_GROUP >= n;
            a.acc_in = g0 ? acc : nullptr;
            a.acc_out = last ? nullptr : acc;
            a.dst = last ? dst : nullptr;
            a.bytes = bytes;
            a.round = n / 2; a.shift = shutter_log2(n);
            shutter_reduce_lin(a, st);
        }
        return;
    }
    unsigned short *acc = n > SHUTTER_GROUP ? (unsigned short *)(S.base + SHUTTER_GROUP * F) + mis : nullptr;
    for (uint32_t g0 = 0; g0 < n; g0 += SHUTTER_GROUP) {
        ShutterArgs a{};
        a.n_frames = std::min(SHUTTER_GROUP, n - g0);
        for (uint32_t k = 0; k < a.n_frames; k++) {
            unsigned char *frame = S.base + k * F + mis;
            set(values + (size_t)(g0 + k) * n_params);
            render(frame);
            a.frames[k] = frame;
        }
        const bool last = g0 + SHUTTER_GROUP >= n;
        a.acc_in = g0 ? acc : nullptr;
        a.acc_out = last ? nullptr : acc;
        a.dst = last ? dst : nullptr;
        a.bytes = bytes;
        a.round = n / 2; a.shift = shutter_log2(n);
        shutter_reduce(a, st);
    }
}

// Puts the values a back-end had before a shutter call back (host only: the next launch copies them), however the call ends.
template <typename B>
struct ShutterRestore {
    B &b;
    const std::vector<double> saved;
    ~ShutterRestore() { try { if (!saved.empty()) b.set_params(saved.data(), (uint32_t)saved.size()); } catch (...) {} }
};

// What the measurement entry points (maray_hip_time_filter*, maray_hip_time_shutter_reduce*) fill their own sample buffers
// with: every byte 0x5A, or, with MARAY_TIME_RANDOM_BYTES=1 in the environment (read at each call), pseudo-random bytes -- for
// the kernels of linear.hip the two ends of the LDS tables' behaviour: every table read of a wavefront a broadcast, and reads
// spread over all entries.  Throws Error.
void measurement_fill(unsigned char *d_buf, size_t bytes);

// Average ms of the passes that reduce n frames of `bytes` bytes (frames of the scratch's own, whatever they hold):
// HIP events on a stream of the device, `reps` repetitions after one warm-up.
float shutter_time_reduce(int device, size_t bytes, uint32_t n, int reps, uint32_t transfer = MARAY_TRANSFER_NONE);

}   // namespace maray
