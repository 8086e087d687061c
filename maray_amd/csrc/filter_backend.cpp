// filter_backend.cpp — the context behind MARAY_FILTER_TENT (product code; include/maray_hip.h, "reconstruction filter").
//
// A Backend that owns a plain (samples = 1) back-end of the supersampled program and changes nothing in it.  Per row block
// of a call, in bands of output rows: one ordinary launch of the band's sample rows plus halo into the context's scratch,
// then maray_filter_tent<k> (filter.hip) on the same stream.  A band's halo is cut from the image, not from the call: rows
// [y0, y1) read sample rows [k y0 - k/2, k y1 + k/2) clipped to [0, k h), whatever row range, row block or host tile they
// belong to, so the picture does not depend on how it was cut.
// Also the context behind MARAY_TRANSFER_SRGB ("transfer"): the same wrapper with the reduces of linear.hip -- the tent in
// linear light, the box as a kernel of the wrapper's on bands without halo, and the shutter's linear reduce; with samples <= 1
// there is nothing to filter and every launch is the inner back-end's.
// And the context behind MARAY_FILTER_CATROM: the tent's bands with a halo of 3k/2 rows and maray_filter_catrom<k> (catrom.hip).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "filter.hpp"
#include "host_pipe.hpp"
#include "shutter.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

struct FilterBackend final : Backend {
    int device = 0;
    uint32_t k = 2;
    // What turns a band into rows: (TENT, NONE) maray_filter_tent<k>; under MARAY_TRANSFER_SRGB (include/maray_hip.h, "transfer")
    // maray_filter_tent_lin<k> or, for BOX, maray_filter_box_lin<k> on a band without halo.  k = 1 (SRGB only) filters nothing:
    // launches go straight to `inner`, and only the shutter's reduce differs.  (CATROM, NONE): maray_filter_catrom<k>.
    uint32_t filter = MARAY_FILTER_TENT, transfer = MARAY_TRANSFER_NONE;
    bool tent() const { return filter == MARAY_FILTER_TENT; }
    bool catrom() const { return filter == MARAY_FILTER_CATROM; }
    bool lin() const { return transfer == MARAY_TRANSFER_SRGB; }
    Backend *inner = nullptr;           // renders the sample raster: the program's plain context
    std::string name;
    // Samples of one band: 128 MiB, half of the 256 MiB last-level cache.  A band is a ROW pass, a pixel launch and a filter pass
    // one after the other on one stream, about 18 us of launches and tails whatever its height (25 bands of
    // 32 MiB cost chess 4096^2 at k = 4 0.4 ms more than 6 of 128 MiB; one band of 768 MiB no less than those 6).
    // MARAY_FILTER_BAND_ROWS=<output rows> (read once, here) overrides it: A/B runs, and tests that want many bands on a
    // small image.
    size_t band_bytes = (size_t)128 << 20;
    uint32_t band_rows_env = 0;
    unsigned char *scratch = nullptr; size_t scratch_cap = 0;      // a band's samples (+ FILTER_PAD on both sides): the context's, ordered by the stream
    unsigned char *d_rgb8 = nullptr; size_t rgb8_cap = 0;           // time_rows without a caller's buffer
    hipStream_t last_stream = nullptr; bool have_last = false;
    hipEvent_t handover = nullptr;
    std::unique_ptr<HostPipe> pipe;     // streams + staging of the host-raster entry points
    std::vector<double> param_values;   // what set_params had last (NaN until set): put back after a shutter call
    ShutterScratch shutter;

    ~FilterBackend() override {
        (void)hipSetDevice(device);
        if (pipe) (void)hipStreamSynchronize(pipe->compute_stream());
        (void)hipFree(scratch); (void)hipFree(d_rgb8);      // (hipFree waits for whatever still reads them)
        shutter.release();
        if (handover) (void)hipEventDestroy(handover);
        if (pipe) host_pipe_release(std::move(pipe));
        delete inner;
    }

    void init(int dev, uint32_t samples, uint32_t n_params) {
        device = dev; k = samples;
        if (const char *e = getenv("MARAY_FILTER_BAND_ROWS")) if (atoll(e) > 0) band_rows_env = (uint32_t)std::min<long long>(atoll(e), 0x7FFFFFFF);
        HIP_TRY(hipSetDevice(dev));
        pipe = host_pipe_acquire(dev);
        HIP_TRY(hipEventCreateWithFlags(&handover, hipEventDisableTiming));
        param_values.assign(n_params, NAN);
    }

    uint32_t band_rows(uint32_t w) const {
        // whole tiles of the filter kernel; one pass of it takes at most 65535 tiles of rows
        const uint64_t by_budget = band_bytes / ((uint64_t)w * 3 * k * k) / FILTER_TILE_H * FILTER_TILE_H;
        const uint64_t rows = band_rows_env ? band_rows_env : std::max<uint64_t>(FILTER_TILE_H, by_budget);
        return (uint32_t)std::min<uint64_t>(rows, 65535u * (uint64_t)FILTER_TILE_H);        // (the linear kernels loop over tiles: any height)
    }

    static void grow(unsigned char *&p, size_t &cap, size_t want) {
        if (want <= cap) return;
        if (p) HIP_TRY(hipFree(p));
        p = nullptr; cap = 0;
        HIP_TRY(hipMalloc((void **)&p, want));
        cap = want;
    }

    // The rows of `rb` into d8, everything enqueued on `st`.
    void launch(uint32_t w, uint32_t h, const RowBlocks &rb, unsigned char *d8, hipStream_t st) {
        if (!rb.n_rows || !w) return;
        if (!d8) throw Error{MARAY_E_ARG, "null argument"};
        if (k == 1) { inner->render_device(w, h, rb, d8, nullptr, st); return; }
        // the scratch is the context's: a launch on another stream than the last waits for what that one still holds
        if (have_last && st != last_stream) {
            HIP_TRY(hipEventRecord(handover, last_stream));
            HIP_TRY(hipStreamWaitEvent(st, handover, 0));
        }
        last_stream = st; have_last = true;
        const uint32_t sw = k * w, sh = k * h, step = band_rows(w);
        const size_t row_bytes = (size_t)sw * 3;
        const uint32_t block_rows = std::max(1u, std::min(rb.block_rows, rb.n_rows));
        const uint32_t halo = filter_halo(filter, k);       // (the box reads sample rows [k y0, k y1) and no others)
        grow(scratch, scratch_cap, ((size_t)k * std::min(step, block_rows) + 2 * halo) * row_bytes + 2 * FILTER_PAD);
        for (uint32_t r0 = 0; r0 < rb.n_rows; r0 += block_rows) {
            const uint32_t rows = std::min(block_rows, rb.n_rows - r0);
            const uint32_t by0 = rb.y0 + (r0 / block_rows) * rb.block_stride;
            for (uint32_t o0 = by0; o0 < by0 + rows; o0 += step) {
                const uint32_t o1 = std::min(by0 + rows, o0 + step);
                const uint32_t s0 = k * o0 >= halo ? k * o0 - halo : 0, s1 = std::min(sh, k * o1 + halo);
                inner->render_device(sw, sh, RowBlocks::range(s0, s1), scratch + FILTER_PAD, nullptr, st);
                const TentArgs a{scratch + FILTER_PAD, d8 + ((size_t)r0 + (o0 - by0)) * w * 3, w, sw, sh, s0, s1 - s0, o0, o1 - o0};
                if (lin()) filter_lin(filter, k, a, st);
                else if (catrom()) filter_catrom(k, a, st);
                else filter_tent(k, a, st);
            }
        }
    }

    void render_device(uint32_t w, uint32_t h, const RowBlocks &rb, void *d8, void *d64, void *stream) override {
        if (k == 1) { inner->render_device(w, h, rb, d8, d64, stream); return; }       // nothing to reduce: the plain render, f64 planes included
        if (d64) throw Error{MARAY_E_ARG, "a filtered context renders RGB8 only (no f64 planes)"};
        HIP_TRY(hipSetDevice(device));
        launch(w, h, rb, (unsigned char *)d8, (hipStream_t)stream);
    }

    void render_host_tiles(uint32_t w, uint32_t h, const std::vector<RowTile> &tiles, uint32_t row0, uint8_t *rgb8, double *rgb64,
                           const std::function<void(uint32_t, uint32_t)> &done) override {
        if (k == 1) { inner->render_host_tiles(w, h, tiles, row0, rgb8, rgb64, done); return; }
        if (rgb64) throw Error{MARAY_E_ARG, "a filtered context renders RGB8 only (no f64 planes)"};
        HIP_TRY(hipSetDevice(device));
        pipe->run(w, tiles, row0, rgb8, nullptr,
                  [&](const RowBlocks &rb, unsigned char *d8, double *, hipStream_t st) { launch(w, h, rb, d8, st); }, done);
    }

    void set_params(const double *values, uint32_t n) override {
        inner->set_params(values, n);
        param_values.assign(values, values + n);
    }

    // One shutter picture into d8: every frame is a tent-filtered render of its own on `st` (shutter.hpp)
    void launch_shutter(uint32_t w, uint32_t h, const RowBlocks &rb, const double *values, uint32_t n, unsigned char *d8, hipStream_t st) {
        const uint32_t np = (uint32_t)param_values.size();
        if (!np || n == 1) {
            if (np) set_params(values, np);
            launch(w, h, rb, d8, st);
            return;
        }
        shutter_render(shutter, values, n, np, (size_t)rb.n_rows * w * 3, d8, st,
                       [&](const double *row) { set_params(row, np); },
                       [&](unsigned char *frame) { launch(w, h, rb, frame, st); }, transfer);
    }

    void render_device_shutter(uint32_t w, uint32_t h, const RowBlocks &rb, const double *values, uint32_t n, void *d8, void *stream) override {
        HIP_TRY(hipSetDevice(device));
        ShutterRestore<FilterBackend> keep{*this, param_values};
        launch_shutter(w, h, rb, values, n, (unsigned char *)d8, (hipStream_t)stream);
    }

    void render_host_tiles_shutter(uint32_t w, uint32_t h, const std::vector<RowTile> &tiles, uint32_t row0, const double *values, uint32_t n,
                                   uint8_t *rgb8, const std::function<void(uint32_t, uint32_t)> &done) override {
        HIP_TRY(hipSetDevice(device));
        ShutterRestore<FilterBackend> keep{*this, param_values};
        pipe->run(w, tiles, row0, rgb8, nullptr,
                  [&](const RowBlocks &rb, unsigned char *d8, double *, hipStream_t st) { launch_shutter(w, h, rb, values, n, d8, st); }, done);
    }

    // the whole call: launches plus filter
    float time_rows(uint32_t w, uint32_t h, const RowBlocks &rb, void *d8, void *d64, int reps) override {
        if (k == 1) return inner->time_rows(w, h, rb, d8, d64, reps);
        if (d64) throw Error{MARAY_E_ARG, "a filtered context renders RGB8 only (no f64 planes)"};
        HIP_TRY(hipSetDevice(device));
        unsigned char *p8 = (unsigned char *)d8;
        if (!p8) { grow(d_rgb8, rgb8_cap, (size_t)rb.n_rows * w * 3); p8 = d_rgb8; }
        const hipStream_t st = pipe->compute_stream();
        for (int i = 0; i < 3; i++) launch(w, h, rb, p8, st);       // (a geometry's second launch computes the specialised kernels' row order)
        struct Events {
            hipEvent_t e0 = nullptr, e1 = nullptr;
            ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
        } ev;
        HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, st));
        for (int i = 0; i < reps; i++) launch(w, h, rb, p8, st);
        HIP_TRY(hipEventRecord(ev.e1, st));
        HIP_TRY(hipEventSynchronize(ev.e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        return ms / (float)(reps > 0 ? reps : 1);
    }

    const char *kernel_name() const override { return name.c_str(); }
    void launch_counts(uint64_t *row_passes, uint64_t *order_kernels) const override { inner->launch_counts(row_passes, order_kernels); }
    uint64_t refine_count() const override { return inner->refine_count(); }
    uint64_t census_count() const override { return inner->census_count(); }
    size_t debug_guard_words(uint64_t *words, size_t cap, uint32_t *per_rect) override { return inner->debug_guard_words(words, cap, per_rect); }
    size_t debug_census_words(uint64_t *words, size_t cap, uint32_t *per_rect) override { return inner->debug_census_words(words, cap, per_rect); }
    uint64_t cover_count() const override { return inner->cover_count(); }
    size_t debug_cover_words(uint64_t *words, size_t cap, uint32_t *per_rect) override { return inner->debug_cover_words(words, cap, per_rect); }
    uint64_t rowscan_count() const override { return inner->rowscan_count(); }
    uint64_t prepass_count() const override { return inner->prepass_count(); }
    uint64_t deferred_count() override { return inner->deferred_count(); }
    size_t debug_row_words(uint64_t *xb, size_t xcap, uint64_t *rw, size_t rcap, size_t *n_rwords, uint32_t *per_rect, int *used) override {
        return inner->debug_row_words(xb, xcap, rw, rcap, n_rwords, per_rect, used);
    }
    void debug_row_sets(int *set, uint32_t *kept_sets, uint64_t *kept_bytes, uint64_t *budget, uint64_t *held) const override {
        inner->debug_row_sets(set, kept_sets, kept_bytes, budget, held);
    }
};

}   // namespace

Backend *make_filter_backend(int device, Backend *inner, uint32_t k, uint32_t n_params, uint32_t filter, uint32_t transfer)
{
    const bool lin = transfer == MARAY_TRANSFER_SRGB, tent = filter == MARAY_FILTER_TENT, catrom = filter == MARAY_FILTER_CATROM;
    // what has a kernel here: the tent for k = 2, 4, 8; under SRGB also the box, and k = 1 (the shutter's reduce alone);
    // Catmull-Rom for k = 2, 4, 8 without a transfer
    if (!inner || (!lin && transfer != MARAY_TRANSFER_NONE) || (!tent && !(catrom && !lin) && (filter != MARAY_FILTER_BOX || !lin)) ||
        !(filter_samples_ok(k) || (k == 1 && lin && !tent && !catrom)))
        throw Error{MARAY_E_INTERNAL, "filter context: bad arguments"};
    std::unique_ptr<FilterBackend> b(new FilterBackend());
    b->init(device, k, n_params);
    b->filter = filter; b->transfer = transfer;
    b->name = std::string(inner->kernel_name()) +
              (k == 1 ? std::string("+maray_shutter_reduce_lin")
                      : std::string(catrom ? "+maray_filter_catrom" : tent ? "+maray_filter_tent" : "+maray_filter_box") + (lin ? "_lin<" : "<") +
                            std::to_string(k) + ">");
    b->inner = inner;       // (last: a throw above leaves `inner` with the caller)
    return b.release();
}

}   // namespace maray
