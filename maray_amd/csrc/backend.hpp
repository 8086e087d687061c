// backend.hpp — device evaluator interface behind the tape-level ABI (product code).
#pragma once

#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "expr.hpp"
#include "maray_hip.h"

namespace maray {

// The image rows of one launch: n_rows rows in blocks of block_rows consecutive ones, block_stride apart.
// Launch row r is image row y0 + (r / block_rows) * block_stride + r % block_rows; outputs are packed in
// launch-row order.  A contiguous range [y0, y1) is one block: {y0, y1 - y0, y1 - y0, 0}.
struct RowBlocks {
    uint32_t y0, n_rows, block_rows, block_stride;
    static RowBlocks range(uint32_t y0, uint32_t y1) { return RowBlocks{y0, y1 - y0, y1 > y0 ? y1 - y0 : 1u, 0u}; }
};

struct RowTile { uint32_t y0, y1; };      // rows [y0, y1)

struct Backend {
    virtual ~Backend() {}
    // the rows of `rb` into device buffers, enqueued on `stream`, no synchronisation
    virtual void render_device(uint32_t w, uint32_t h, const RowBlocks &rb, void *d8, void *d64, void *stream) = 0;
    // The row tiles, in order, into host rasters whose first byte is image row `row0` (blocking; either raster may
    // be null).  Tile k's device -> host copy runs under tile k + 1's kernels (host_pipe.hpp); `done` (may be empty)
    // is called on this thread once a tile's rows are in the raster.
    virtual void render_host_tiles(uint32_t w, uint32_t h, const std::vector<RowTile> &tiles, uint32_t row0, uint8_t *rgb8, double *rgb64,
                                   const std::function<void(uint32_t, uint32_t)> &done) = 0;
    // average ms per launch of the pixel kernel, HIP events on the launch stream
    virtual float time_rows(uint32_t w, uint32_t h, const RowBlocks &rb, void *d8, void *d64, int reps) = 0;
    virtual const char *kernel_name() const = 0;
    // How many ROW passes (maray_jit_rows) and launch-order kernels (maray_jit_order) the context has enqueued so far: what
    // the tests of the ROW tables' reuse (row_reuse.hpp) count.  The interpreters run their ROW stage per launch and count nothing.
    virtual void launch_counts(uint64_t *row_passes, uint64_t *order_kernels) const { *row_passes = *order_kernels = 0; }
    // maray_jit_refine passes enqueued so far, and (test access) the guard words of the set the last launch used, after a
    // wait for the context's work: returns the words in the set, copies at most `cap` (maray_hip_debug_guard_words)
    virtual uint64_t refine_count() const { return 0; }
    virtual uint64_t census_count() const { return 0; }     // maray_jit_census launches enqueued so far (maray_hip_census_count)
    virtual size_t debug_guard_words(uint64_t *, size_t, uint32_t *) { throw Error{MARAY_E_ARG, "this context keeps no guard words"}; }
    // ... and the words the last launch read: those with the bits its set's census cleared, where it has been through one (maray_hip_debug_census_words)
    virtual size_t debug_census_words(uint64_t *, size_t, uint32_t *) { throw Error{MARAY_E_ARG, "this context keeps no guard words"}; }
    // maray_jit_cover launches enqueued so far (maray_hip_cover_count), and the words the last launch read, cover bits included
    // where it ran maray_jit_pixels_cov (maray_hip_debug_cover_words)
    virtual uint64_t cover_count() const { return 0; }
    virtual size_t debug_cover_words(uint64_t *, size_t, uint32_t *) { throw Error{MARAY_E_ARG, "this context keeps no guard words"}; }
    // maray_jit_rowscan launches enqueued so far (maray_hip_rowscan_count), and the fourth table and the row words of the set the
    // last launch used (maray_hip_debug_row_words): returns the words of xbits and *n_rwords, copies at most the caps; 0 and 0 for
    // a set that has been through no row scan
    virtual uint64_t rowscan_count() const { return 0; }
    // launches of maray_jit_pixels_pp enqueued so far (maray_hip_prepass_count)
    virtual uint64_t prepass_count() const { return 0; }
    // tiles the most recent launch deferred to the interpreter (maray_hip_deferred_count, test access); waits for the context's work
    virtual uint64_t deferred_count() { return 0; }
    virtual size_t debug_row_words(uint64_t *, size_t, uint64_t *, size_t, size_t *, uint32_t *, int *) { throw Error{MARAY_E_ARG, "this context keeps no guard words"}; }
    // The kept sets of ROW tables (maray_hip_debug_row_sets): the set the last launch used (-1 before any), how many sets are
    // kept, the bytes accounted to them, the budget, and the device bytes their tables hold.  Host state only: no wait.
    virtual void debug_row_sets(int *, uint32_t *, uint64_t *, uint64_t *, uint64_t *) const { throw Error{MARAY_E_ARG, "this context keeps no sets of ROW tables"}; }
    // The values of the program's parameters (n = its count, every value inside its range: checked by the caller) for the
    // launches enqueued after this call; kept on the host until then.  A launch copies changed values to the device on its
    // own stream, in front of its ROW pass.
    virtual void set_params(const double *, uint32_t) { throw Error{MARAY_E_INTERNAL, "this program has no parameters"}; }
    // Shutter (include/maray_hip.h, "shutter"): the integer mean of the n RGB8 frames that the rows of `values` (n x the
    // program's parameter count, frame-major, every value inside its range: checked by the caller; null for a program
    // without parameters) render, n in {1, 2, 4, ..., 64}.  Per frame set_params(row) and the ordinary launch into the
    // context's scratch, per group of 8 frames one pass of maray_shutter_reduce on the same stream (shutter.hpp); the
    // values set_params had before the call are put back (on the host) before it returns.
    virtual void render_device_shutter(uint32_t w, uint32_t h, const RowBlocks &rb, const double *values, uint32_t n, void *d8, void *stream) = 0;
    virtual void render_host_tiles_shutter(uint32_t w, uint32_t h, const std::vector<RowTile> &tiles, uint32_t row0, const double *values, uint32_t n,
                                           uint8_t *rgb8, const std::function<void(uint32_t, uint32_t)> &done) = 0;
    // Tape interpreter only: re-evaluate the 256-pixel tiles of the device work list
    // {count, tile, tile, ...} (tile = row_in_launch * ceil(w/256) + x/256), reading the row
    // values from `yvals` instead of running the ROW section.  Enqueued on `stream`.
    virtual void render_flagged(uint32_t, const RowBlocks &, void *, void *, void *, const unsigned *, const double *) {
        throw Error{MARAY_E_INTERNAL, "render_flagged is not supported by this backend"};
    }
};

// host_pipe.cpp: rows [y0, y1) of a w-wide image cut into tiles of a few MiB of output; pinned host memory
std::vector<RowTile> cut_row_tiles(uint32_t w, uint32_t y0, uint32_t y1, bool want8, bool want64);
void *host_alloc_pinned(size_t bytes);          // throws Error
void host_free_pinned(void *p);
void host_register(void *p, size_t bytes);      // throws Error
void host_unregister(void *p);                  // throws Error
bool host_range_is_pinned(const void *p, size_t n);

void set_last_error(const std::string &m);   // thread-local message behind maray_last_error()
int read_whole_file(const char *path, std::vector<uint8_t> &b);                                             // png.cpp; MARAY_E_IO + message on failure
int png_decode(const std::vector<uint8_t> &b, uint8_t **rgb8_out, uint32_t *w_out, uint32_t *h_out);       // png.cpp
int hip_device_count();
// samples = k > 1: a supersampling context (maray_ctx_opts.samples): renders RGB8 only, geometry in output pixels
Backend *make_tape_backend(int device, const maray_program &prog, const maray_texture *tex, uint32_t n_tex, bool lds_variant, uint32_t samples = 1);
// refine: the program's REFINE section (null or empty: none), evaluated behind every ROW pass (maray_jit_refine)
Backend *make_jit_backend(int device, const maray_program &prog, const maray_texture *tex, uint32_t n_tex, uint32_t samples = 1, const maray_refine *refine = nullptr);
std::string jit_source(const maray_program &prog, int min_waves = 0);   // PIXEL kernel source (__launch_bounds__(256, min_waves); 0 = the layout's default); throws Error
std::string jit_source_rows(const maray_program &prog, uint32_t *n_chunks_out = nullptr, uint32_t *n_gjobs_out = nullptr);   // ROW kernel source (blockIdx.y = chunk)
// How the specialised kernels keep a program's guards (test access, maray_jit_guard_layout): pos[g] = the bit of guard g (y value
// numeric_yvals + g) in a rectangle's words, -1 for a guard derived from others' bits; words per rectangle (0: guards not kept as
// bits) and the rectangle, in pixels x rows
void jit_guard_layout(const maray_program &prog, std::vector<int32_t> &pos, uint32_t *n_words, uint32_t *gw, uint32_t *gh);
// maray_jit_refine: the REFINE section on the rectangles whose guard bits are set; "" when there is nothing to launch.  *n_jobs_out: blockIdx.y of its launch
std::string jit_source_refine(const maray_program &prog, const maray_refine &refine, uint32_t *n_jobs_out = nullptr);
// its code object (null when the source is empty): built once, kept like jit_code_samples', under a key of its own made of its text
struct JitRefineCode { std::vector<char> code; uint32_t n_jobs = 0; };
std::shared_ptr<const JitRefineCode> jit_code_refine(const maray_program &prog, const maray_refine &refine);
// maray_jit_census + maray_jit_census_apply: the census form of the PIXEL kernel (which guarded leaves are != 0 on some pixel of
// a rectangle) and the kernel that clears the guard bits of the others; "" when no bit is eligible.  *eligible: per guard word, the
// bits a census decides (maray_jit_census_eligible)
std::string jit_source_census(const maray_program &prog, std::vector<uint64_t> *eligible = nullptr, int min_waves = 0);
// its code object (null when the source is empty): a module and a cache entry of its own, like jit_code_refine's
struct JitCensusCode { std::vector<char> code; std::vector<uint64_t> eligible; };
std::shared_ptr<const JitCensusCode> jit_code_census(const maray_program &prog);
// The cover bits of a program (maray_jit_cover_bits): per boolean reduction the census may decide, one free bit of the last
// guard word that says "this OR of shapes is 1 on every pixel of the rectangle"; its guarded leaves (their last op, their guard
// bit, tainted: not counted by the measurement, eligible: cleared where the cover bit is set)
struct CoverPlan {
    struct Red { int32_t bit = -1; uint32_t root = 0; std::vector<uint32_t> leaf_end, leaf_bit; std::vector<uint8_t> leaf_taint, leaf_eligible; };
    std::vector<Red> reds;
    uint32_t n_words = 0;               // guard words per rectangle
};
CoverPlan jit_cover_plan(const maray_program &prog);
// maray_jit_pixels_cov + maray_jit_cover + maray_jit_cover_apply (one module); "" when the program gets no cover bit
std::string jit_source_cover(const maray_program &prog, CoverPlan *plan = nullptr, int min_waves = 0);
// its code object (null when the source is empty): a module and a cache entry of its own (<key>.mrcv), like jit_code_census'
struct JitCoverCode { std::vector<char> code; uint32_t n_cover = 0; };      // n_cover: reductions with a bit (2 flag bytes each per rectangle)
std::shared_ptr<const JitCoverCode> jit_code_cover(const maray_program &prog);
// The row words of a program (jit_source.cpp, "maray_jit_rowscan"): flag_bit = the free bit of the last guard word that says "this
// rectangle's words are taken per row" (-1: the program gets no row words), the words per rectangle and the reductions with a cover bit
struct RowWordsPlan { int32_t flag_bit = -1; uint32_t n_words = 0, n_cover = 0; };
RowWordsPlan jit_rowwords_plan(const maray_program &prog);
// maray_jit_pixels_rw + maray_jit_rowscan (one module); "" when the program gets no row words
std::string jit_source_rowwords(const maray_program &prog, RowWordsPlan *plan = nullptr, int min_waves = 0);
// its code object (null when the source is empty): a module and a cache entry of its own (<key>.mrrw), like jit_code_cover's.  Built by the
// first launch that wants it, never when a context is created
struct JitRowWordsCode { std::vector<char> code; int32_t flag_bit = -1; };
std::shared_ptr<const JitRowWordsCode> jit_code_rowwords(const maray_program &prog);
// maray_jit_pixels_pp (jit_source.cpp): maray_jit_pixels_rw with a wide pre-pass of a busy tile's leafless rectangles; "" when
// the program gets none (no row words, or a cover bit outside the last guard word)
std::string jit_source_prepass(const maray_program &prog, int min_waves = 0);
// its code object (null when the source is empty): a module and a cache entry of its own (<key>.mrpp), built beside jit_code_rowwords'
struct JitPrepassCode { std::vector<char> code; };
std::shared_ptr<const JitPrepassCode> jit_code_prepass(const maray_program &prog);
std::string jit_source_samples(const maray_program &prog, uint32_t k, int min_waves = 0);   // supersampling PIXEL kernel (maray_jit_pixels_ss), k = 2, 4, 8
std::shared_ptr<const std::vector<char>> jit_code_samples(const maray_program &prog, uint32_t k);   // its code object: built once, kept like jit_code_for's
void jit_compile(const std::string &src, std::vector<char> &code, std::string &log);     // hiprtc, gfx950; throws Error
// The two code objects of a program (jit_build.cpp): built once per process, kept on disk under MARAY_CACHE_DIR.
struct JitCode {
    std::vector<char> pix, rows;        // maray_jit_pixels; maray_jit_rows + maray_jit_order (empty without a ROW section)
    uint32_t n_row_chunks = 1, n_gjobs = 0;
    uint32_t n_gwords = 0, guard_w = 256, guard_h = 1;      // guard words per rectangle and the rectangle they are bounded over (what the sources were generated for)
    int waves = 8;                      // the __launch_bounds__ occupancy the PIXEL kernel was built for
    bool from_disk = false;
};
std::shared_ptr<const JitCode> jit_code_for(const maray_program &prog);      // needs no GPU; throws Error
std::string jit_code_key(const maray_program &prog);                        // 128-bit hash (hex) of generated sources + toolchain: the cache's file name
bool jit_code_is_cached(const maray_program &prog);                         // in this process or on disk: no hiprtc build needed
void validate_program(const maray_program &p);
maray_program load_program(const maray_program *p);

// The interpreter's view of a program with parameters: PARAM p is the constant n_consts + p of a pool that ends in the
// parameters' values (NaN until set), so that its kernels -- generic loop, pre-decoded loop, LDS staging -- read a
// parameter as the wave-uniform table entry a constant is, unchanged.  A version-2 program in every other respect.
struct ParamsAsConsts {
    std::vector<double> consts;
    std::vector<uint64_t> row_ops, pix_ops;
    maray_program prog;                 // points into this object
    explicit ParamsAsConsts(const maray_program &P);
    ParamsAsConsts(const ParamsAsConsts &) = delete;
};

// Parameter values on their way to the device: pinned host slots, so that a launch's copy is asynchronous and several
// frames can be in flight.  A slot is reused once the copy that read it has completed (an event per slot).
struct ParamRing {
    static constexpr int SLOTS = 8;
    double *host = nullptr;
    void *events[SLOTS] = {};
    uint32_t n = 0;
    int next = 0;
    void init(uint32_t n_params);       // throws Error
    double *take();                     // the next free slot (waits for its last copy, if that is still in flight)
    void sent(void *stream);            // the slot take() returned is being read by a copy enqueued on `stream`
    void release();
};

// ---- ROW-tape analysis shared by the evaluators (row_split.cpp) ------------------------------------
// Number of leading y values that PIXEL ops read as arithmetic operands; the rest of the table only gates SKIP ops.
uint32_t numeric_yvals(const maray_program &P);
struct RowTapeDeps {
    std::vector<std::array<int32_t, 2>> deps;   // per op: the ops that produce its operands (-1: none)
    std::vector<uint32_t> outs;                 // OUT ops, tape order
    std::vector<uint8_t> reads_y;               // per op: SPEC Y is somewhere in its cone
};
RowTapeDeps row_tape_deps(const maray_program &P);
// The ROW tape with everything but the cone of the given OUT ops turned into NOPs (SKIP regions kept when their end is).
std::vector<uint64_t> row_tape_cone(const maray_program &P, const RowTapeDeps &d, const std::vector<uint32_t> &outs, size_t *cost);
// The same tape without its NOPs (SKIP op counts adjusted).
std::vector<uint64_t> compact_tape(const std::vector<uint64_t> &tape);
// Renumbers the value slots of a compacted tape by liveness; returns the number of slots it then uses.
uint32_t renumber_slots(std::vector<uint64_t> &tape);
uint32_t reschedule_tape(std::vector<uint64_t> &tape);   // cone re-ordered depth first + slots by liveness
// Does any guard (a y value that only gates SKIP ops) have SPEC Y in its cone?  If none does, guards may be evaluated
// once for a group of rows (YMIN / YMAX, include/maray_tape.h).
bool any_guard_reads_y(const maray_program &P);
// Bit p is set when an op of the ROW section has PARAM p as an operand: the parameters whose values the ROW outputs (y values,
// guard bits) depend on.  0 for a program without parameters.
uint64_t row_param_mask(const maray_program &P);

}   // namespace maray

struct maray_ctx {
    maray::Backend *backend = nullptr;
    uint32_t n_tex = 0;
    uint32_t samples = 1;       // maray_ctx_opts.samples (0 taken as 1)
    std::vector<double> param_ranges;   // lo, hi per parameter of the program: what maray_hip_ctx_set_params enforces
    // Every parameter starts as NaN, which only the range (-inf, +inf) admits: a program with any other range renders once
    // its values have been set (what the lowering proved from a finite range does not hold for NaN).
    bool params_ready = true;
};
