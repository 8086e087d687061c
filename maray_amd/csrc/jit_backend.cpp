// jit_backend.cpp — the specialised kernels of a program on one device (product code): code objects -> modules, tables,
// launches.  The GPU analogue of the reference's
//
//   JitBackend   <- wasm_par_gen_to_image                         src/render.rs:102-192
//
// The sources come from jit_source.cpp, the code objects from jit_build.cpp (jit_parts.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "host_pipe.hpp"
#include "jit_parts.hpp"
#include "maray_hip.h"
#include "row_reuse.hpp"
#include "rowwords.hpp"
#include "shutter.hpp"

namespace maray {


namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

struct DevTex { const unsigned char *rgb; unsigned w, h; };

// The device memory of one set of ROW-stage tables (row_reuse.hpp has the sets' keys and decides which one a launch uses)
struct RowTables {
    double *yvals = nullptr; size_t yvals_cap = 0;
    unsigned long long *gbits = nullptr; size_t gbits_cap = 0;
    unsigned *order = nullptr; size_t order_cap = 0;          // the launch order computed from gbits (maray_jit_order)
    unsigned char *hits = nullptr; size_t hits_cap = 0;       // the census's flags, 64 per guard word (maray_jit_census)
    unsigned long long *cbits = nullptr; size_t cbits_cap = 0;      // gbits with the bits the census cleared: what the launches of a set read once it is through (maray_jit_census_apply)
    unsigned long long *vbits = nullptr; size_t vbits_cap = 0;      // cbits with cover bits in place of the leaves of ORs that are 1 on every pixel of a rectangle (maray_jit_cover_apply)
    unsigned char *cflags = nullptr; size_t cflags_cap = 0;         // the cover's flags, 2 per rectangle and reduction with a bit (maray_jit_cover)
    unsigned long long *rwords = nullptr; size_t rwords_cap = 0;    // the words of every (row, rectangle): the band's words refined on that row (maray_jit_rowscan); read only for flagged rectangles
    unsigned char *changed = nullptr; size_t changed_cap = 0;       // per rectangle and row of its band: the row's words differ from the band's
    unsigned long long *xbits = nullptr; size_t xbits_cap = 0;      // vbits (cbits for a program without cover bits) with the row flag of the rectangles that take their words per row (maray_jit_rowscan_apply)
    void release() {
        (void)hipFree(yvals); (void)hipFree(gbits); (void)hipFree(order); (void)hipFree(hits); (void)hipFree(cbits); (void)hipFree(vbits); (void)hipFree(cflags);
        (void)hipFree(rwords); (void)hipFree(changed); (void)hipFree(xbits);
        *this = RowTables{};
    }
};

struct JitBackend final : Backend {
    int device = 0;
    maray_program P{};
    std::shared_ptr<const JitCode> code;
    hipModule_t mod = nullptr, mod_rows = nullptr;
    hipFunction_t f_rows = nullptr, f_pix = nullptr, f_order = nullptr;
    // maray_jit_refine (the program's REFINE section, jit_source_refine): behind every ROW pass, into the same guard words
    std::shared_ptr<const JitRefineCode> code_refine;
    hipModule_t mod_refine = nullptr;
    hipFunction_t f_refine = nullptr;
    bool refine_on = true;              // MARAY_JIT_GUARD_REFINE=0: no such launch (read once, when the context is created)
    uint64_t n_refine_passes = 0;
    // maray_jit_census + maray_jit_census_apply (jit_source_census): once per kept filling of a set, in front of its launch order
    std::shared_ptr<const JitCensusCode> code_census;
    hipModule_t mod_census = nullptr;
    hipFunction_t f_census = nullptr, f_census_apply = nullptr;
    bool census_on = true;              // MARAY_JIT_GUARD_CENSUS=0: no such launch (read once, when the context is created)
    uint64_t n_census = 0;
    // the census module's parameter table is not among d_par: it is written by the launch that takes a census, not by every
    // frame of an animation (a copy per module and frame is what a host-bound shutter waits for)
    hipDeviceptr_t d_par_census = nullptr;
    // maray_jit_cover + maray_jit_cover_apply + maray_jit_pixels_cov (jit_source_cover): the cover is taken once per kept filling
    // of a set, behind its census; a set in which it set at least one bit is rendered by maray_jit_pixels_cov over vbits
    std::shared_ptr<const JitCoverCode> code_cover;
    hipModule_t mod_cover = nullptr;
    hipFunction_t f_cover = nullptr, f_cover_apply = nullptr, f_pix_cov = nullptr;
    bool cover_on = true;               // MARAY_JIT_GUARD_COVER=0: none of this (read once, when the context is created; in no code key)
    uint64_t n_cover = 0;
    // How many cover bits a set's apply kernel set: counted on the device, copied behind the kernel into pinned memory and read
    // by the first later launch that finds the copy complete (an event per set, queried, never waited for).  Until then, and
    // when the count is 0, the set's launches are what they were: maray_jit_pixels over cbits.
    enum CoverState : uint8_t { COVER_NONE = 0, COVER_PENDING, COVER_SOME, COVER_EMPTY };
    CoverState cover_state[RowReuse::N_SETS] = {};
    hipEvent_t cover_ev[RowReuse::N_SETS] = {};
    unsigned *d_cover_n = nullptr, *h_cover_n = nullptr;     // one word per set
    // the cover module's parameter table: written when it is behind the values a launch of one of its kernels renders with
    hipDeviceptr_t d_par_cover = nullptr;
    uint64_t par_serial = 1, par_cover_serial = 0;
    bool last_cov = false;              // the most recent launch ran maray_jit_pixels_cov over vbits (or maray_jit_pixels_rw over a covered set's xbits: vbits with row flags)
    // maray_jit_rowscan + maray_jit_pixels_rw (jit_source_rowwords) and maray_jit_rowscan_apply (rowwords.hip): the row scan is taken
    // once per kept filling of a set, behind its cover; a set in which the apply kernel flagged at least one rectangle is rendered
    // by maray_jit_pixels_rw over xbits and rwords.  The module is built and loaded by the first launch that is due a scan
    // (rowwords_module): a context's creation and a one-shot render never pay for it.
    std::shared_ptr<const JitRowWordsCode> code_rw;
    hipModule_t mod_rw = nullptr;
    hipFunction_t f_rowscan = nullptr, f_pix_rw = nullptr;
    bool rw_on = true;                  // MARAY_JIT_ROW_WORDS=0: none of this (read once, when the context is created; in no code key)
    bool rw_asked = false;              // the module has been asked for (whether or not the program gets one)
    unsigned rw_threshold = 0;          // MARAY_ROW_WORDS_T: changed rows from which a rectangle is flagged (0: a quarter of the band's rows); a measurement knob
    uint64_t n_rowscan = 0;
    CoverState rw_state[RowReuse::N_SETS] = {};      // the flag count of a set's apply kernel, like the cover's count
    hipEvent_t rw_ev[RowReuse::N_SETS] = {};
    unsigned *d_rw_n = nullptr, *h_rw_n = nullptr;          // one word per set
    size_t set_rw_n[RowReuse::N_SETS] = {};         // row words each set's last scan covered
    hipDeviceptr_t d_par_rw = nullptr;
    uint64_t par_rw_serial = 0;
    bool last_rw = false;               // the most recent launch ran maray_jit_pixels_rw (or maray_jit_pixels_pp over a set with row words)
    // maray_jit_pixels_pp (jit_source_prepass): maray_jit_pixels_rw with a wide pre-pass of a busy tile's leafless rectangles.  Asked
    // for beside the row-word module (rowwords_module); where it is in place it takes the launches of maray_jit_pixels_cov (over
    // vbits: no row flag is set there, so no row word is read) and of maray_jit_pixels_rw (over xbits and rwords)
    std::shared_ptr<const JitPrepassCode> code_pp;
    hipModule_t mod_pp = nullptr;
    hipFunction_t f_pix_pp = nullptr;
    bool pp_on = true;                  // MARAY_JIT_PREPASS=0: none of this (read once, when the context is created; in no code key)
    uint64_t n_prepass = 0;             // launches that ran maray_jit_pixels_pp
    hipDeviceptr_t d_par_pp = nullptr;
    uint64_t par_pp_serial = 0;
    // the program, kept for the lazy build (P's arrays are not the context's to keep)
    std::vector<double> own_consts, own_ranges;
    std::vector<uint64_t> own_row_ops, own_pix_ops;
    uint32_t ss = 1;                    // samples per output pixel and axis: > 1 launches maray_jit_pixels_ss (launch_ss)
    std::shared_ptr<const std::vector<char>> code_ss;
    hipModule_t mod_ss = nullptr;
    hipFunction_t f_ss = nullptr;
    Backend *slow = nullptr;            // tape interpreter: evaluates the tiles the pixel kernel deferred
    unsigned *d_flags = nullptr; size_t flags_cap = 0;
    DevTex *d_tex = nullptr;
    std::vector<unsigned char *> d_tex_rgb;
    // ROW-stage tables (the context's, not a launch's: launches are ordered by their stream): set 0 is the scratch every
    // one-off launch fills, the others are kept for keys that came back (row_reuse.hpp)
    RowTables tabs[RowReuse::N_SETS];
    RowReuse reuse;
    int cur_set = -1;                   // the set the most recent launch used
    size_t set_gbits_n[RowReuse::N_SETS] = {};      // guard words each set's last ROW pass wrote
    size_t last_gbits_n = 0;            // ... and the most recent launch's
    uint64_t row_params = 0;            // bit p: a ROW op reads PARAM p (row_param_mask)
    uint64_t n_row_passes = 0, n_order_kernels = 0;         // maray_jit_rows / maray_jit_order launches enqueued so far (launch_counts)
    unsigned char *d_rgb8 = nullptr; size_t rgb8_cap = 0;      // time_rows without a caller's buffer
    std::unique_ptr<HostPipe> pipe;     // streams + staging of the host-raster entry points (from the device's pool: host_pipe.hpp)
    hipStream_t own_stream = nullptr;   // = pipe's compute stream
    uint32_t n_row_chunks = 1, n_gwords = 0, n_gjobs = 0, guard_rows = 1, guard_sub = 1;       // guard_sub: guard rectangles per 256-pixel tile
    uint32_t n_cu = 256;
    bool wide_all = false;              // the whole section runs four pixels per lane (jit_wide_general)
    unsigned k_tiles = 0;               // MARAY_JIT_TILES: tiles per wavefront (0 = by launch size), read once when the context is created
    bool has_sin = false;               // some Sin argument is not proven bounded: tiles may be deferred to `slow`
    hipStream_t last_stream = nullptr; bool have_last = false;      // the stream of the last launch (see launch())
    hipEvent_t handover = nullptr;
    // Parameters: the table `mr_par_tab` of every module of the program (PIXEL, ROW, supersampling); values wait on the host
    // (set_params) for the next launch, which copies them on its stream in front of its ROW pass (send_params)
    std::vector<hipDeviceptr_t> d_par;
    std::vector<double> param_values;
    bool params_dirty = false;
    ParamRing ring;
    ShutterScratch shutter;             // frames and partial sums of the shutter entry points (shutter.hpp)

    ~JitBackend() override {
        (void)hipSetDevice(device);
        delete slow;
        if (mod) (void)hipModuleUnload(mod);
        if (mod_rows) (void)hipModuleUnload(mod_rows);
        if (mod_refine) (void)hipModuleUnload(mod_refine);
        if (mod_census) (void)hipModuleUnload(mod_census);
        if (mod_cover) (void)hipModuleUnload(mod_cover);
        if (mod_rw) (void)hipModuleUnload(mod_rw);
        if (mod_pp) (void)hipModuleUnload(mod_pp);
        for (hipEvent_t e : rw_ev) if (e) (void)hipEventDestroy(e);
        (void)hipFree(d_rw_n);
        if (h_rw_n) (void)hipHostFree(h_rw_n);
        for (hipEvent_t e : cover_ev) if (e) (void)hipEventDestroy(e);
        (void)hipFree(d_cover_n);
        if (h_cover_n) (void)hipHostFree(h_cover_n);
        if (mod_ss) (void)hipModuleUnload(mod_ss);
        (void)hipFree(d_flags);
        (void)hipFree(d_tex);
        for (auto p : d_tex_rgb) (void)hipFree(p);
        (void)hipFree(d_rgb8);
        for (RowTables &t : tabs) t.release();
        shutter.release();
        if (handover) (void)hipEventDestroy(handover);
        ring.release();
        if (pipe) { (void)hipStreamSynchronize(pipe->compute_stream()); host_pipe_release(std::move(pipe)); }
    }

    void init(int dev, const maray_program &prog, const maray_texture *tex, uint32_t n_tex, uint32_t samples, const maray_refine *refine) {
        device = dev;
        ss = samples;
        // MARAY_TRACE_INIT=1: where the time of a context's creation goes (stderr)
        const bool trace = getenv("MARAY_TRACE_INIT") && getenv("MARAY_TRACE_INIT")[0] == '1';
        auto t_last = std::chrono::steady_clock::now();
        auto lap = [&](const char *what) {
            if (!trace) return;
            const auto now = std::chrono::steady_clock::now();
            fprintf(stderr, "maray init: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
            t_last = now;
        };
        HIP_TRY(hipSetDevice(dev));
        // (hipGetDeviceProperties costs ~5 ms a call: asked once per device and process)
        static std::mutex prop_mutex;
        static std::map<int, std::pair<std::string, int>> props;
        std::pair<std::string, int> info;
        {
            std::lock_guard<std::mutex> lk(prop_mutex);
            auto it = props.find(dev);
            if (it == props.end()) {
                hipDeviceProp_t prop;
                HIP_TRY(hipGetDeviceProperties(&prop, dev));
                it = props.emplace(dev, std::make_pair(std::string(prop.gcnArchName), prop.multiProcessorCount)).first;
            }
            info = it->second;
        }
        if (info.first.rfind("gfx950", 0) != 0)
            throw Error{MARAY_E_NO_DEVICE, "device is " + info.first + ", this library is built for gfx950 only"};
        n_cu = (uint32_t)std::max(1, info.second);
        has_sin = may_defer_tiles(prog);
        // (set below, from the code object's header: the guard plan is not recomputed per context)
        if (const char *e_ = getenv("MARAY_JIT_TILES")) if (atoi(e_) > 0) k_tiles = (unsigned)atoi(e_);
        // MARAY_JIT_ROW_REUSE=0: a ROW pass per launch and one set of tables, as before the sets had keys (read once, here)
        if (const char *e_ = getenv("MARAY_JIT_ROW_REUSE")) if (e_[0] == '0') reuse.enabled = false;
        row_params = row_param_mask(prog);
        lap("device");
        if (const char *e_ = getenv("MARAY_JIT_GUARD_REFINE")) if (e_[0] == '0') refine_on = false;
        // the third module is asked for first, on a thread of its own: a cold start builds the three side by side
        std::future<std::shared_ptr<const JitRefineCode>> refine_code;
        if (refine_on && refine && refine->n_ops && prog.n_row_ops)
            refine_code = std::async(std::launch::async, [&prog, refine] { return jit_code_refine(prog, *refine); });
        // ... and the fourth: a plain context that reuses its sets (a supersampling context takes no census)
        if (const char *e_ = getenv("MARAY_JIT_GUARD_CENSUS")) if (e_[0] == '0') census_on = false;
        std::future<std::shared_ptr<const JitCensusCode>> census_code;
        if (census_on && reuse.enabled && ss == 1 && prog.n_row_ops)
            census_code = std::async(std::launch::async, [&prog] { return jit_code_census(prog); });
        // ... and the fifth, wherever a census is taken
        if (const char *e_ = getenv("MARAY_JIT_GUARD_COVER")) if (e_[0] == '0') cover_on = false;
        std::future<std::shared_ptr<const JitCoverCode>> cover_code;
        if (cover_on && census_code.valid())
            cover_code = std::async(std::launch::async, [&prog] { return jit_code_cover(prog); });
        try { code = jit_code_for(prog); }               // built by the first context of the process, or read from the cache
        catch (...) { if (refine_code.valid()) refine_code.wait(); if (census_code.valid()) census_code.wait(); if (cover_code.valid()) cover_code.wait(); throw; }
        try { if (refine_code.valid()) code_refine = refine_code.get(); }
        catch (...) { if (census_code.valid()) census_code.wait(); if (cover_code.valid()) cover_code.wait(); throw; }
        try { if (census_code.valid()) code_census = census_code.get(); }
        catch (...) { if (cover_code.valid()) cover_code.wait(); throw; }
        if (cover_code.valid()) code_cover = cover_code.get();
        lap("code objects");
        HIP_TRY(hipModuleLoadData(&mod, code->pix.data()));
        HIP_TRY(hipModuleGetFunction(&f_pix, mod, "maray_jit_pixels"));
        lap("load PIXEL module");
        n_row_chunks = code->n_row_chunks; n_gjobs = code->n_gjobs;
        wide_all = jit_wide_general(prog, code->n_gwords);
        if (ss > 1) {               // the supersampling kernel defers nothing: no interpreter behind it
            code_ss = jit_code_samples(prog, ss);
            HIP_TRY(hipModuleLoadData(&mod_ss, code_ss->data()));
            HIP_TRY(hipModuleGetFunction(&f_ss, mod_ss, "maray_jit_pixels_ss"));
            lap("load supersampling PIXEL module");
        } else if (has_sin) slow = make_tape_backend(dev, prog, tex, n_tex, false);     // drains the tiles the pixel kernel defers; other programs never defer
        P = prog;
        P.consts = nullptr; P.row_ops = nullptr; P.pix_ops = nullptr;
        if (const char *e_ = getenv("MARAY_JIT_ROW_WORDS")) if (e_[0] == '0') rw_on = false;
        if (const char *e_ = getenv("MARAY_JIT_PREPASS")) if (e_[0] == '0') pp_on = false;
        // two hooks for tests and measurements, taken only when the whole string is a number in range: the threshold of
        // maray_jit_rowscan_apply (1 .. 128 rows), and the byte budget of the kept sets, row words included (row_reuse.hpp)
        auto number = [](const char *name, unsigned long long lo, unsigned long long hi, unsigned long long *v) {
            const char *e_ = getenv(name);
            if (!e_ || !e_[0]) return false;
            char *end = nullptr;
            const unsigned long long x = strtoull(e_, &end, 10);
            if (*end || e_[0] == '-' || x < lo || x > hi) return false;
            *v = x;
            return true;
        };
        unsigned long long knob = 0;
        if (number("MARAY_ROW_WORDS_T", 1, 128, &knob)) rw_threshold = (unsigned)knob;
        if (number("MARAY_ROW_KEPT_BYTES", 0, (unsigned long long)RowReuse::MAX_BYTES, &knob)) reuse.max_bytes = (size_t)knob;
        if (prog.n_row_ops) {
            HIP_TRY(hipModuleLoadData(&mod_rows, code->rows.data()));
            HIP_TRY(hipModuleGetFunction(&f_rows, mod_rows, "maray_jit_rows"));
            n_gwords = code->n_gwords;
            if (n_gwords) HIP_TRY(hipModuleGetFunction(&f_order, mod_rows, "maray_jit_order"));
            guard_rows = code->guard_h;
            guard_sub = 256u / code->guard_w;
            lap("load ROW module");
            if (code_refine && n_gwords) {
                HIP_TRY(hipModuleLoadData(&mod_refine, code_refine->code.data()));
                HIP_TRY(hipModuleGetFunction(&f_refine, mod_refine, "maray_jit_refine"));
                lap("load REFINE module");
            }
            if (code_census && n_gwords && code_census->eligible.size() == n_gwords) {
                HIP_TRY(hipModuleLoadData(&mod_census, code_census->code.data()));
                HIP_TRY(hipModuleGetFunction(&f_census, mod_census, "maray_jit_census"));
                HIP_TRY(hipModuleGetFunction(&f_census_apply, mod_census, "maray_jit_census_apply"));
                lap("load CENSUS module");
            }
            if (code_cover && f_census) {
                HIP_TRY(hipModuleLoadData(&mod_cover, code_cover->code.data()));
                HIP_TRY(hipModuleGetFunction(&f_cover, mod_cover, "maray_jit_cover"));
                HIP_TRY(hipModuleGetFunction(&f_cover_apply, mod_cover, "maray_jit_cover_apply"));
                HIP_TRY(hipModuleGetFunction(&f_pix_cov, mod_cover, "maray_jit_pixels_cov"));
                HIP_TRY(hipMalloc((void **)&d_cover_n, RowReuse::N_SETS * sizeof(unsigned)));
                HIP_TRY(hipHostMalloc((void **)&h_cover_n, RowReuse::N_SETS * sizeof(unsigned), hipHostMallocDefault));
                lap("load COVER module");
            }
            // row words: wherever a census is taken, for rectangles one pass wide whose words are fetched per strip; the program is
            // kept for the module's build, which the first launch that is due a scan asks for
            if (rw_on && f_census && guard_sub == 4 && n_gwords <= GW_INLINE_MAX && guard_rows > 1) {
                own_consts.assign(prog.consts, prog.consts + prog.n_consts);
                own_row_ops.assign(prog.row_ops, prog.row_ops + prog.n_row_ops);
                own_pix_ops.assign(prog.pix_ops, prog.pix_ops + prog.n_pix_ops);
                if (prog.n_params && prog.param_ranges) own_ranges.assign(prog.param_ranges, prog.param_ranges + 2 * (size_t)prog.n_params);
            } else rw_on = false;
        }
        if (prog.n_params) {
            param_values.assign(prog.n_params, NAN);
            for (hipModule_t m : {mod, mod_rows, mod_ss, mod_refine, mod_census, mod_cover}) {
                if (!m) continue;
                hipDeviceptr_t p = nullptr;
                size_t bytes = 0;
                HIP_TRY(hipModuleGetGlobal(&p, &bytes, m, "mr_par_tab"));
                if (bytes != (size_t)prog.n_params * sizeof(double)) throw Error{MARAY_E_INTERNAL, "parameter table of a module has another size than the program"};
                HIP_TRY(hipMemcpyHtoD(p, param_values.data(), bytes));          // NaN until set
                if (m == mod_census) d_par_census = p; else if (m == mod_cover) d_par_cover = p; else d_par.push_back(p);
            }
            ring.init(prog.n_params);
            P.param_ranges = nullptr;
        }
        pipe = host_pipe_acquire(dev);
        lap("host pipe");
        own_stream = pipe->compute_stream();
        HIP_TRY(hipEventCreateWithFlags(&handover, hipEventDisableTiming));
        std::vector<DevTex> descs(n_tex ? n_tex : 1);
        for (uint32_t i = 0; i < n_tex; i++) {
            unsigned char *d = nullptr;
            const size_t bytes = (size_t)tex[i].w * tex[i].h * 3;
            HIP_TRY(hipMalloc((void **)&d, bytes ? bytes : 8));
            if (bytes) HIP_TRY(hipMemcpy(d, tex[i].rgb, bytes, hipMemcpyHostToDevice));
            d_tex_rgb.push_back(d);
            descs[i] = DevTex{d, tex[i].w, tex[i].h};
        }
        HIP_TRY(hipMalloc((void **)&d_tex, descs.size() * sizeof(DevTex)));
        HIP_TRY(hipMemcpy(d_tex, descs.data(), descs.size() * sizeof(DevTex), hipMemcpyHostToDevice));
        lap("streams, events, textures");
    }

    template <typename T>
    void ensure(T *&p, size_t &cap, size_t n) {
        if (n <= cap) return;
        if (p) HIP_TRY(hipFree(p));
        p = nullptr; cap = 0;
        HIP_TRY(hipMalloc((void **)&p, n * sizeof(T)));
        cap = n;
    }

    void set_params(const double *values, uint32_t n) override {
        if (n != param_values.size()) throw Error{MARAY_E_INTERNAL, "parameter count"};
        if (slow) slow->set_params(values, n);          // the interpreter that drains deferred tiles renders the same frame
        if (memcmp(param_values.data(), values, (size_t)n * sizeof(double)) == 0) return;       // the same bits: nothing to send
        param_values.assign(values, values + n);
        params_dirty = true;
    }

    // New values reach the tables on the launch's own stream: launches enqueued before the set_params call keep theirs.
    // Every changed value is sent -- the PIXEL module reads them all -- and nothing is dropped here: what depends on the
    // values carries them in its key.  Three things read a geometry's ROW outputs; with new values:
    //  - the ROW tables themselves (y values, guard bits): keyed on the geometry and on the bits of the values the ROW
    //    section reads (row_params), so a change to one of those is another key -- its launch finds no set and runs the ROW
    //    pass -- and a change to a parameter only PIXEL ops read is the same key: no ROW pass.  A launch without a ROW
    //    pass of its own (time_rows) that carries new values asks for one (the return value says so) and gets it only
    //    if no set holds the key.
    //  - the launch order: a permutation of rows from the guard bits of one set, kept in that set and so under the same
    //    key; computed when a key comes a second time (a paused animation, a benchmark loop, an animation of PIXEL-only
    //    parameters), never per frame of one whose ROW-read values move: the order kernel costs more than ten launches'
    //    gain.
    //  - deferred tiles: the interpreter behind this context has the values already (set_params) and sends them on the
    //    same stream, in front of its kernel; it reads the y values of the set the launch used.
    bool send_params(hipStream_t st) {
        if (!params_dirty) return false;
        double *slot = ring.take();
        const size_t bytes = param_values.size() * sizeof(double);
        memcpy(slot, param_values.data(), bytes);
        for (hipDeviceptr_t p : d_par) HIP_TRY(hipMemcpyHtoDAsync(p, slot, bytes, st));
        ring.sent(st);
        params_dirty = false;
        par_serial++;
        return true;
    }

    // the cover module's table, in front of a launch of one of its kernels on `st`, if it is behind the context's values
    void send_params_cover(hipStream_t st) {
        if (!d_par_cover || par_cover_serial == par_serial) return;
        double *slot = ring.take();
        const size_t bytes = param_values.size() * sizeof(double);
        memcpy(slot, param_values.data(), bytes);
        HIP_TRY(hipMemcpyHtoDAsync(d_par_cover, slot, bytes, st));
        ring.sent(st);
        par_cover_serial = par_serial;
    }

    // the row-word module's table, likewise
    void send_params_rw(hipStream_t st) {
        if (!d_par_rw || par_rw_serial == par_serial) return;
        double *slot = ring.take();
        const size_t bytes = param_values.size() * sizeof(double);
        memcpy(slot, param_values.data(), bytes);
        HIP_TRY(hipMemcpyHtoDAsync(d_par_rw, slot, bytes, st));
        ring.sent(st);
        par_rw_serial = par_serial;
    }

    // the pre-pass module's table, likewise
    void send_params_pp(hipStream_t st) {
        if (!d_par_pp || par_pp_serial == par_serial) return;
        double *slot = ring.take();
        const size_t bytes = param_values.size() * sizeof(double);
        memcpy(slot, param_values.data(), bytes);
        HIP_TRY(hipMemcpyHtoDAsync(d_par_pp, slot, bytes, st));
        ring.sent(st);
        par_pp_serial = par_serial;
    }

    // The pre-pass module, from the build rowwords_module started beside the row-word module's.  A build or a load that fails
    // leaves the context on maray_jit_pixels_cov / maray_jit_pixels_rw and says so once on stderr.
    void prepass_module(std::future<std::shared_ptr<const JitPrepassCode>> &build) {
        hipModule_t m = nullptr;
        try {
            std::shared_ptr<const JitPrepassCode> c = build.get();
            if (!c) return;                             // the program gets none
            hipFunction_t fp = nullptr;
            hipDeviceptr_t par = nullptr;
            HIP_TRY(hipModuleLoadData(&m, c->code.data()));
            HIP_TRY(hipModuleGetFunction(&fp, m, "maray_jit_pixels_pp"));
            if (P.n_params) {
                size_t bytes = 0;
                HIP_TRY(hipModuleGetGlobal(&par, &bytes, m, "mr_par_tab"));
                if (bytes != (size_t)P.n_params * sizeof(double)) throw Error{MARAY_E_INTERNAL, "parameter table of a module has another size than the program"};
            }
            code_pp = c; mod_pp = m; f_pix_pp = fp; d_par_pp = par;
            par_pp_serial = 0;
        } catch (const Error &e) {
            if (m) (void)hipModuleUnload(m);
            (void)hipGetLastError();
            fprintf(stderr, "maray: no pre-pass kernel for this context (launches go on without it): %s\n", e.msg.c_str());
        } catch (const std::exception &e) {            // (out of the build's thread: no memory, no thread)
            if (m) (void)hipModuleUnload(m);
            fprintf(stderr, "maray: no pre-pass kernel for this context (launches go on without it): %s\n", e.what());
        }
    }

    // The row-word module: built (a helper process, or read from the cache) and loaded by the first launch that is due a row
    // scan -- that launch waits for it; until then, and for a program that gets none, launches are what they were.  Asked for
    // once.  The context's handles are set only when everything is in place; a build or a load that fails leaves the context
    // without row words -- the launch that asked goes on as it would with the knob off, and says so once on stderr (the
    // module is an optimisation of launches that are correct without it: a render must not fail where knob-off succeeds).
    void rowwords_module() {
        if (rw_asked) return;
        rw_asked = true;
        hipModule_t m = nullptr;
        unsigned *dn = nullptr, *hn = nullptr;
        try {
            maray_program Q = P;
            Q.consts = own_consts.data(); Q.row_ops = own_row_ops.data(); Q.pix_ops = own_pix_ops.data();
            Q.param_ranges = own_ranges.empty() ? nullptr : own_ranges.data();
            // the pre-pass module beside it: two helper processes, one wait
            std::future<std::shared_ptr<const JitPrepassCode>> pp_build;
            if (pp_on) pp_build = std::async(std::launch::async, [&Q] { return jit_code_prepass(Q); });
            std::shared_ptr<const JitRowWordsCode> c;
            try { c = jit_code_rowwords(Q); }
            catch (...) { if (pp_build.valid()) pp_build.wait(); throw; }
            if (!c || (uint32_t)c->flag_bit / 64 != n_gwords - 1) { if (pp_build.valid()) pp_build.wait(); rw_on = false; return; }       // the program gets none
            hipFunction_t fs = nullptr, fp = nullptr;
            hipDeviceptr_t par = nullptr;
            HIP_TRY(hipModuleLoadData(&m, c->code.data()));
            HIP_TRY(hipModuleGetFunction(&fs, m, "maray_jit_rowscan"));
            HIP_TRY(hipModuleGetFunction(&fp, m, "maray_jit_pixels_rw"));
            if (P.n_params) {
                size_t bytes = 0;
                HIP_TRY(hipModuleGetGlobal(&par, &bytes, m, "mr_par_tab"));
                if (bytes != (size_t)P.n_params * sizeof(double)) throw Error{MARAY_E_INTERNAL, "parameter table of a module has another size than the program"};
            }
            HIP_TRY(hipMalloc((void **)&dn, RowReuse::N_SETS * sizeof(unsigned)));
            HIP_TRY(hipHostMalloc((void **)&hn, RowReuse::N_SETS * sizeof(unsigned), hipHostMallocDefault));
            code_rw = c; mod_rw = m; f_rowscan = fs; f_pix_rw = fp; d_rw_n = dn; h_rw_n = hn; d_par_rw = par;
            par_rw_serial = 0;          // behind whatever the context holds: sent in front of the module's first kernel
            if (pp_build.valid()) prepass_module(pp_build);
        } catch (const Error &e) {
            if (hn) (void)hipHostFree(hn);
            (void)hipFree(dn);
            if (m) (void)hipModuleUnload(m);
            (void)hipGetLastError();
            rw_on = false;
            fprintf(stderr, "maray: no row words for this context (launches go on without them): %s\n", e.msg.c_str());
        }
    }

    // The set of ROW tables a launch reads, filled by maray_jit_rows on `st` unless a set already holds the outputs of this
    // launch's key: the geometry and the bits of the ROW-read parameters (with MARAY_JIT_ROW_REUSE=0 of all parameters, and
    // a launch that asks for a ROW pass runs it whatever the tables hold).  rows_pass == false never runs the kernel: the
    // set that holds the key, else the set of the previous launch as it is.  *matched: the set holds this launch's key.
    // Called after the stream hand-over and send_params: every launch of the context is ordered behind the previous one,
    // whichever streams they are on, so a set filled on one stream is complete for a reader on another.
    int row_set(uint32_t w, uint32_t rows_total, unsigned y0, unsigned blk_rows, unsigned blk_stride, unsigned yrows, uint32_t n_groups,
                bool want_order, hipStream_t st, bool rows_pass, bool *matched, bool want_census = false) {
        RowKey key;
        key.geometry(w, rows_total, y0, blk_rows, blk_stride, yrows);
        key.params(param_values.data(), (uint32_t)param_values.size(), reuse.enabled ? row_params : ~0ull);
        int s = reuse.find(key);
        *matched = true;
        if (s >= 0 && (reuse.enabled || !rows_pass)) {
            reuse.touch(s);
            last_gbits_n = set_gbits_n[s];
            return cur_set = s;
        }
        if (!rows_pass) {
            if (cur_set < 0) throw Error{MARAY_E_INTERNAL, "launch without a ROW pass before any ROW pass"};
            *matched = false;
            return cur_set;
        }
        const size_t yv_n = (size_t)rows_total * std::max<uint32_t>(P.n_yvals, 1);
        const size_t gb_n = (size_t)n_groups * ((w + 255) / 256) * guard_sub * std::max<uint32_t>(n_gwords, 1);
        const size_t od_n = want_order ? rows_total : 0;
        const size_t hb_n = want_census ? gb_n * 64 : 0;           // a flag per guard bit
        const size_t cb_n = want_census ? gb_n : 0;                // ... and the words the census leaves
        const size_t vb_n = want_census && f_cover ? gb_n : 0;     // ... and the cover; its flags
        const size_t cf_n = vb_n ? gb_n / std::max<uint32_t>(n_gwords, 1) * 2 * code_cover->n_cover : 0;
        const bool refill = s >= 0;             // reuse is off: the scratch holds this key and is written again
        if (!refill)
            s = reuse.place(key, yv_n * sizeof(double) + gb_n * sizeof(unsigned long long) + od_n * sizeof(unsigned) + hb_n + cb_n * sizeof(unsigned long long) + vb_n * sizeof(unsigned long long) + cf_n,
                            [&](int v) { return tabs[v].yvals_cap >= yv_n && tabs[v].gbits_cap >= gb_n && tabs[v].order_cap >= od_n && tabs[v].hits_cap >= hb_n && tabs[v].cbits_cap >= cb_n &&
                                                tabs[v].vbits_cap >= vb_n && tabs[v].cflags_cap >= cf_n; },
                            [&](int v) { tabs[v].release(); });      // (hipFree waits for the device: at a promotion or an eviction only)
        RowTables &t = tabs[s];
        ensure(t.yvals, t.yvals_cap, yv_n);
        const size_t had = t.gbits_cap;
        ensure(t.gbits, t.gbits_cap, gb_n);
        // A kept set gets its order table with the other two, whether or not an order is ever computed in it: fits() asks for
        // all three, so a set whose keys rotate away before their second launch can still be taken over as it is (the
        // scratch's grows in launch(), when an order is due)
        if (s) { ensure(t.order, t.order_cap, od_n); ensure(t.hits, t.hits_cap, hb_n); ensure(t.cbits, t.cbits_cap, cb_n); ensure(t.vbits, t.vbits_cap, vb_n); ensure(t.cflags, t.cflags_cap, cf_n); }      // (the census's flags likewise)
        // bits past the last guard belong to no job and are never written: zero them once per table (the pixel kernel tests whole words)
        if (t.gbits_cap != had) HIP_TRY(hipMemsetAsync(t.gbits, 0, t.gbits_cap * sizeof(unsigned long long), st));
        if (P.n_row_ops) {
            unsigned rr = rows_total, ww = w, n_yvals = P.n_yvals;
            unsigned n_tx_ = (w + 255) / 256 * guard_sub;
            // guards: one item per rectangle (group of yrows rows, run of 256 / guard_sub pixels); y values: one per row
            const uint64_t items = std::max<uint64_t>(n_gwords ? (uint64_t)n_groups * n_tx_ : 0, rows_total);
            const unsigned bs = ROW_BLOCK;
            if (items + bs > 0xFFFFFFFFull) throw Error{MARAY_E_ARG, "too many tiles in one launch; render fewer rows per call"};
            void *args[] = {&t.yvals, &t.gbits, &d_tex, &y0, &rr, &n_yvals, &ww, &n_tx_, &blk_rows, &blk_stride, &yrows};
            unsigned gy = n_row_chunks + n_gjobs;
            HIP_TRY(hipModuleLaunchKernel(f_rows, (unsigned)((items + bs - 1) / bs), gy, 1, bs, 1, 1, 0, st, args, nullptr));
            n_row_passes++;
            // the second bounds, into the words the ROW pass has just written: in front of the launch order, which counts
            // the bits that are left, and of every reader (one stream)
            if (f_refine && n_gwords) {
                void *rargs[] = {&t.gbits, &d_tex, &y0, &rr, &ww, &n_tx_, &blk_rows, &blk_stride, &yrows};
                const uint64_t rects = (uint64_t)n_groups * n_tx_;
                HIP_TRY(hipModuleLaunchKernel(f_refine, (unsigned)((rects + bs - 1) / bs), code_refine->n_jobs, 1, bs, 1, 1, 0, st, rargs, nullptr));
                n_refine_passes++;
            }
        }
        cover_state[s] = COVER_NONE;
        rw_state[s] = COVER_NONE;
        if (refill) reuse.touch(s); else reuse.filled(s);      // the set carries its key only now: the kernel that fills it is enqueued
        last_gbits_n = set_gbits_n[s] = gb_n;
        return cur_set = s;
    }

    // Supersampling (maray_jit_pixels_ss): w_out and rb_out are output pixels and rows; the ROW stage covers the k x k times
    // larger sample grid, the PIXEL kernel's grid counts output rows (65,534 per grid).  No launch order, nothing deferred.
    void launch_ss(uint32_t w_out, const RowBlocks &rb_out, unsigned char *d8, hipStream_t st, bool rows_pass) {
        const uint32_t w = w_out * ss;
        const RowBlocks rb{rb_out.y0 * ss, rb_out.n_rows * ss, rb_out.block_rows * ss, rb_out.block_stride * ss};
        const uint32_t rows_total = rb.n_rows;
        unsigned y0 = rb.y0, blk_rows = rb.block_rows, blk_stride = rb.block_stride;
        if (!rows_total || !w) return;
        if (have_last && st != last_stream) {
            HIP_TRY(hipEventRecord(handover, last_stream));
            HIP_TRY(hipStreamWaitEvent(st, handover, 0));
        }
        last_stream = st; have_last = true;
        if (send_params(st)) rows_pass = true;
        unsigned yrows = (guard_rows > 1 && (blk_rows >= rows_total || blk_rows % guard_rows == 0)) ? guard_rows : 1u;
        const uint32_t n_groups = (rows_total + yrows - 1) / yrows;
        bool matched;
        const RowTables &T = tabs[row_set(w, rows_total, y0, blk_rows, blk_stride, yrows, n_groups, false, st, rows_pass, &matched)];   // keyed on the sample grid
        if (!T.yvals || !T.gbits) throw Error{MARAY_E_INTERNAL, "launch without a ROW pass before any ROW pass"};
        unsigned n_yvals = P.n_yvals;
        // tiles per wavefront: the narrow rule of launch(), on the tiles of sample rows a launch evaluates
        const unsigned n_tx = (w + 255) / 256;
        const uint64_t n_tiles = (uint64_t)n_tx * rows_total, device_slots = (uint64_t)n_cu * 4 * 7;
        unsigned tiles = n_tiles <= 4 * device_slots ? 1 : n_tiles <= 16 * device_slots ? 2 : 4;
        if (k_tiles) tiles = std::min(64u, k_tiles);
        tiles = std::max(1u, std::min(tiles, n_tx));
        const unsigned gx = (n_tx + 4 * tiles - 1) / (4 * tiles);
        for (uint32_t r0 = 0; r0 < rb_out.n_rows; r0 += 65534u) {
            const uint32_t rows = std::min<uint32_t>(65534u, rb_out.n_rows - r0);
            unsigned ww = w, row_base = r0, ntx = n_tx, wo = w_out;
            const double *yv = T.yvals;
            const unsigned long long *gb = T.gbits;
            void *args[] = {&d8, &yv, &d_tex, &gb, &ntx, &ww, &y0, &n_yvals, &tiles, &blk_rows, &blk_stride, &row_base, &yrows, &wo};
            HIP_TRY(hipModuleLaunchKernel(f_ss, gx, rows, 1, 256, 1, 1, 0, st, args, nullptr));
        }
    }

    void launch(uint32_t w, const RowBlocks &rb, unsigned char *d8, double *d64, hipStream_t st, bool rows_pass) {
        if (ss > 1) {
            if (d64) throw Error{MARAY_E_INTERNAL, "supersampling renders RGB8 only"};
            launch_ss(w, rb, d8, st, rows_pass);
            return;
        }
        const uint32_t rows_total = rb.n_rows, y0 = rb.y0;
        unsigned blk_rows = rb.block_rows, blk_stride = rb.block_stride;
        if (!rows_total || !w) return;
        // The scratch tables (y values, guard bits, row order, work list) belong to the context, not to a launch: launches
        // are ordered by the stream they are issued on.  When a launch arrives on another stream than the last one, that
        // stream is made to wait for everything the previous one holds (one event, only at the hand-over).
        if (have_last && st != last_stream) {
            HIP_TRY(hipEventRecord(handover, last_stream));
            HIP_TRY(hipStreamWaitEvent(st, handover, 0));
        }
        last_stream = st; have_last = true;
        if (send_params(st)) rows_pass = true;
        // rows per guard evaluation: a group must not straddle two row blocks (its image rows have to be consecutive)
        unsigned yrows = (guard_rows > 1 && (blk_rows >= rows_total || blk_rows % guard_rows == 0)) ? guard_rows : 1u;
        const uint32_t n_groups = (rows_total + yrows - 1) / yrows;
        // (the ROW stage on a stream of its own under the previous launch's PIXEL kernel was measured and lost: the two kernels
        // share the SIMDs and the events that order the streams cost a signal round trip each)
        const uint32_t rows_per_grid = 65534u;                         // gridDim.y limit (an even number of rows: whole 32-row groups)
        // the launch order is a permutation of the launch's rows and every grid reads it from its first entry: a launch of
        // more than one grid takes none
        const bool want_order = f_order && n_gwords && rows_total <= rows_per_grid && n_groups <= 4096 && n_groups > 1;
        bool matched;
        // the census is a launch of the pixel kernel's shape over the set's geometry: a launch of more than one grid takes none
        const bool want_census = f_census && rows_total <= rows_per_grid;
        const int set = row_set(w, rows_total, y0, blk_rows, blk_stride, yrows, n_groups, want_order, st, rows_pass, &matched, want_census);
        RowTables &T = tabs[set];
        if (!T.yvals || !T.gbits) throw Error{MARAY_E_INTERNAL, "launch without a ROW pass before any ROW pass"};
        unsigned n_yvals = P.n_yvals;
        const unsigned n_tx = (w + 255) / 256;
        const uint64_t n_tiles = (uint64_t)n_tx * rows_total;
        // Tiles per wavefront.  Every tile of a program without guards costs the same: nothing to balance, and a strip as long as
        // the launch is deep -- a wavefront's tiles come one after the other, so a launch that fills the device once is as
        // long as its longest strip (config 2, RGB8, us per frame with 1 / 2 / 4 / 8 / 16 tiles: 1024^2 3.03 / 3.14 / 3.53 (whole
        // rows); 2048^2 6.86 / 6.70 / 6.99 / 7.63; 4096^2 19.4 / 18.4 / 18.4 / 21.5 / 20.2; 8192^2 65.7 / 63.0 / 63.0 / 60.1 / 69.5; only
        // for the cheap four-wide sections, a narrow wavefront would live too long).  Else rows cost what they show (sky: nothing, board: 5x the average) and wavefronts are the unit of load
        // balance: a launch that fills the device only a few times over -- chess up to 2048^2 -- is a matter of how long its
        // longest wavefront lives, not of throughput: one tile per wavefront (1024^2 / 2048^2 / 4096^2 / 8192^2 with 1 tile:
        // 20.3 / 18.9 / 48.4 / 149 us per step, with 2: 25.5 / 24.8 / 42.3 / 138); a launch that fills it dozens of times over
        // is a matter of what every wavefront costs before its first pixel, its tail is short against the whole: four tiles
        // (8192^2 / 16384^2 with 2 / 3 / 4 / 5 tiles: 138 / 123 / 119 / 139 and 517 / 487 / 497 / 566 us per step; 4096^2:
        // 42.2 / 55.5 / 44.6 / 46.9)
        const uint64_t device_slots = (uint64_t)n_cu * 4 * 7;
        unsigned tiles = wide_all ? (n_tiles <= device_slots ? 1 : n_tiles <= 4 * device_slots ? 2 : n_tiles <= 16 * device_slots ? 4 : 8)
                                  : (n_tiles <= 4 * device_slots ? 1 : n_tiles <= 16 * device_slots ? 2 : 4);
        if (k_tiles) tiles = std::min(64u, k_tiles);
        if (n_gwords && n_gwords <= GW_INLINE_MAX) tiles = std::min(tiles, 64u / (n_gwords * guard_sub));      // a strip's guard words: one per lane
        tiles = std::max(1u, std::min(tiles, n_tx));
        const unsigned gx = (n_tx + 4 * tiles - 1) / (4 * tiles);
        if (n_tiles > 0xFFFFFFFFull) throw Error{MARAY_E_ARG, "too many tiles in one launch; render fewer rows per call"};
        // The census (maray_jit_census, jit_source_census): the pixel launch without its stores, over exactly the set's geometry,
        // records which leaves are != 0 on some pixel of each rectangle; maray_jit_census_apply writes the set's guard words without the
        // eligible bits of the others into the set's second table, cbits, which this launch and the later ones read.  Once per filling of a set, on the first launch that finds it filled (row_reuse.hpp,
        // census_due) -- its inputs are the program, the geometry and the ROW-read parameters, a set's key -- and in front of the
        // launch order, which counts the bits that are left.  One stream: flags zeroed, census, apply, order, pixels.
        if (want_census && reuse.census_due(set, matched)) {
            const size_t words = set_gbits_n[set];
            if (words && words <= 0xFFFFFFFFull / 64) {
                ensure(T.hits, T.hits_cap, words * 64);
                ensure(T.cbits, T.cbits_cap, words);
                HIP_TRY(hipMemsetAsync(T.hits, 0, words * 64, st));
                if (d_par_census) {             // the values this launch renders with (send_params has run)
                    double *slot = ring.take();
                    const size_t bytes = param_values.size() * sizeof(double);
                    memcpy(slot, param_values.data(), bytes);
                    HIP_TRY(hipMemcpyHtoDAsync(d_par_census, slot, bytes, st));
                    ring.sent(st);
                }
                unsigned char *no8 = nullptr; double *no64 = nullptr; unsigned *fl = nullptr; const unsigned *no_order = nullptr;
                const double *yv = T.yvals;
                const unsigned long long *gb = T.gbits;
                unsigned ww = w, yy0 = y0, tile_base = 0, row_base = 0, ntx = n_tx, rows = rows_total, rpw = 1;
                unsigned char *hits = T.hits;
                void *cargs[] = {&no8, &no64, &yv, &d_tex, &fl, &tile_base, &gb, &ntx, &ww, &yy0, &n_yvals, &tiles, &blk_rows, &blk_stride, &row_base, &yrows, &no_order, &rows, &rpw, &hits};
                HIP_TRY(hipModuleLaunchKernel(f_census, gx, rows_total, 1, 256, 1, 1, 0, st, cargs, nullptr));
                unsigned long long *cbw = T.cbits;
                unsigned nw = (unsigned)words;
                void *aargs[] = {&gb, &hits, &cbw, &nw};
                HIP_TRY(hipModuleLaunchKernel(f_census_apply, (nw + 255u) / 256u, 1, 1, 256, 1, 1, 0, st, aargs, nullptr));
                n_census++;
                reuse.sets[set].census = true;          // only now: the kernels are enqueued
            }
        }
        // The cover (maray_jit_cover, jit_source_cover): the census's launch over the census'd words records per rectangle which ORs
        // of shapes are 1 on every pixel; maray_jit_cover_apply writes the set's third table, vbits.  Behind the census's apply
        // kernel, in front of the launch order, on this stream; once per filling of a set.
        if (want_census && f_cover && reuse.cover_due(set, matched)) {
            const size_t words = set_gbits_n[set], rects = words / n_gwords, flags = rects * 2 * code_cover->n_cover;
            if (words && words <= 0xFFFFFFFFull / 64) {
                ensure(T.vbits, T.vbits_cap, words);
                ensure(T.cflags, T.cflags_cap, flags);
                if (!cover_ev[set]) HIP_TRY(hipEventCreateWithFlags(&cover_ev[set], hipEventDisableTiming));
                HIP_TRY(hipMemsetAsync(T.cflags, 0, flags, st));
                HIP_TRY(hipMemsetAsync(d_cover_n + set, 0, sizeof(unsigned), st));
                send_params_cover(st);
                unsigned char *no8 = nullptr; double *no64 = nullptr; unsigned *fl = nullptr; const unsigned *no_order = nullptr;
                const double *yv = T.yvals;
                const unsigned long long *cb = T.cbits;
                unsigned ww = w, yy0 = y0, tile_base = 0, row_base = 0, ntx = n_tx, rows = rows_total, rpw = 1;
                unsigned char *cf = T.cflags;
                void *cargs[] = {&no8, &no64, &yv, &d_tex, &fl, &tile_base, &cb, &ntx, &ww, &yy0, &n_yvals, &tiles, &blk_rows, &blk_stride, &row_base, &yrows, &no_order, &rows, &rpw, &cf};
                HIP_TRY(hipModuleLaunchKernel(f_cover, gx, rows_total, 1, 256, 1, 1, 0, st, cargs, nullptr));
                unsigned long long *vb = T.vbits;
                unsigned nw = (unsigned)words;
                unsigned *cnt = d_cover_n + set;
                void *aargs[] = {&cb, &cf, &vb, &nw, &cnt};
                HIP_TRY(hipModuleLaunchKernel(f_cover_apply, (nw + 255u) / 256u, 1, 1, 256, 1, 1, 0, st, aargs, nullptr));
                HIP_TRY(hipMemcpyAsync(h_cover_n + set, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipEventRecord(cover_ev[set], st));
                n_cover++;
                cover_state[set] = COVER_PENDING;
                reuse.sets[set].cover = true;           // only now: the kernels are enqueued
            }
        }
        // has the count of a cover taken by an earlier launch arrived?  (a query: nothing waits)
        if (reuse.sets[set].cover && cover_state[set] == COVER_PENDING && matched) {
            const hipError_t q = hipEventQuery(cover_ev[set]);
            if (q == hipSuccess) cover_state[set] = h_cover_n[set] ? COVER_SOME : COVER_EMPTY;
            else if (q == hipErrorNotReady) (void)hipGetLastError();      // not an error: the status is not left behind as HIP's last one
            else HIP_TRY(q);
        }
        // The row scan (maray_jit_rowscan, jit_source_rowwords): the cover's launch once more, over the words the cover left (the
        // census's for a program without cover bits), forms every (rectangle, row)'s own words; maray_jit_rowscan_apply flags the
        // rectangles where enough rows differ from the band, in the set's fourth table, xbits.  Behind the cover's apply kernel on
        // this stream, once per filling of a set; its tables count against the kept sets' budget and a set they do not fit takes
        // none.  Not for launches whose guard groups are one row high.
        if (rw_on && want_census && yrows > 1 && reuse.rowwords_due(set, matched, f_cover != nullptr)) {
            rowwords_module();
            const size_t words = set_gbits_n[set], rects = words / std::max<uint32_t>(n_gwords, 1);
            const size_t rw_n = (size_t)rows_total * (rects / n_groups) * n_gwords, ch_n = rects * yrows;
            if (f_rowscan && words && words <= 0xFFFFFFFFull / 64 && rects <= 0xFFFFFFFFull &&
                reuse.rowwords_admit(set, (rw_n + words) * sizeof(unsigned long long) + ch_n)) {
                ensure(T.rwords, T.rwords_cap, rw_n);
                ensure(T.changed, T.changed_cap, ch_n);
                ensure(T.xbits, T.xbits_cap, words);
                if (!rw_ev[set]) HIP_TRY(hipEventCreateWithFlags(&rw_ev[set], hipEventDisableTiming));
                HIP_TRY(hipMemsetAsync(T.changed, 0, ch_n, st));
                HIP_TRY(hipMemsetAsync(d_rw_n + set, 0, sizeof(unsigned), st));
                send_params_rw(st);
                unsigned char *no8 = nullptr; double *no64 = nullptr; unsigned *fl = nullptr; const unsigned *no_order = nullptr;
                const double *yv = T.yvals;
                const unsigned long long *src = reuse.sets[set].cover ? T.vbits : T.cbits;
                unsigned ww = w, yy0 = y0, tile_base = 0, row_base = 0, ntx = n_tx, rows = rows_total, rpw = 1;
                unsigned long long *rwp = T.rwords;
                unsigned char *chp = T.changed;
                void *sargs[] = {&no8, &no64, &yv, &d_tex, &fl, &tile_base, &src, &ntx, &ww, &yy0, &n_yvals, &tiles, &blk_rows, &blk_stride, &row_base, &yrows, &no_order, &rows, &rpw, &rwp, &chp};
                HIP_TRY(hipModuleLaunchKernel(f_rowscan, gx, rows_total, 1, 256, 1, 1, 0, st, sargs, nullptr));
                const unsigned threshold = rw_threshold ? rw_threshold : std::max(1u, yrows / 4u);
                HIP_TRY((hipError_t)rowwords_apply_launch(src, T.changed, T.xbits, (unsigned)rects, n_gwords, yrows, threshold,
                                                          1ull << ((uint32_t)code_rw->flag_bit % 64), d_rw_n + set, (void *)st));
                HIP_TRY(hipMemcpyAsync(h_rw_n + set, d_rw_n + set, sizeof(unsigned), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipEventRecord(rw_ev[set], st));
                n_rowscan++;
                set_rw_n[set] = rw_n;
                rw_state[set] = COVER_PENDING;
            }
            if (rw_asked) reuse.sets[set].rowwords = true;       // only now: the kernels are enqueued (or the set takes none: its state stays COVER_NONE)
        }
        if (reuse.sets[set].rowwords && rw_state[set] == COVER_PENDING && matched) {
            const hipError_t q = hipEventQuery(rw_ev[set]);
            if (q == hipSuccess) rw_state[set] = h_rw_n[set] ? COVER_SOME : COVER_EMPTY;
            else if (q == hipErrorNotReady) (void)hipGetLastError();
            else HIP_TRY(q);
        }
        const bool use_rw = f_pix_rw && matched && reuse.sets[set].rowwords && rw_state[set] == COVER_SOME;
        const bool use_cov = !use_rw && f_pix_cov && matched && reuse.sets[set].cover && cover_state[set] == COVER_SOME;
        // launch order of the PIXEL kernel (maray_jit_order): once per key, from the set's guard bits, whether this launch
        // ran the ROW kernel or found them there; used by every later launch of that key (time_rows too)
        // the guard words this launch and its order read: the census's where the set has been through one
        const unsigned long long *gwords = use_rw ? T.xbits : use_cov ? T.vbits : reuse.sets[set].census ? T.cbits : T.gbits;
        // (the order reads the words this launch reads: vbits only for a set whose apply kernel is known to have set a bit)
        const unsigned long long *owords = gwords;
        const bool use_pp = f_pix_pp && (use_rw || use_cov);
        // (the table of the module whose kernel this launch runs, and of no other)
        if (use_pp) { send_params_pp(st); n_prepass++; }
        else if (use_cov) send_params_cover(st);
        else if (use_rw) send_params_rw(st);
        last_cov = use_cov || (use_rw && reuse.sets[set].cover);
        last_rw = use_rw;
        const unsigned *row_order = nullptr;
        if (want_order && matched) {
            RowReuse::Set &S = reuse.sets[set];
            // The order costs one 43 us kernel per key and saves ~2.6 us per launch: it is computed by the first launch that
            // finds the set holding its key (an animation, a benchmark loop: the second launch; a key that came back into
            // a kept set: the launch after the one that filled it), never for the tiles of a one-shot render, each of
            // which is a geometry of its own, nor for keys that rotate through more sets than a context keeps.
            if (!S.order && S.launches >= 2) {
                ensure(T.order, T.order_cap, (size_t)rows_total);
                unsigned rr = rows_total, n_tx_ = (w + 255) / 256 * guard_sub;
                void *oargs[] = {&owords, &T.order, &rr, &n_tx_, &yrows};
                HIP_TRY(hipModuleLaunchKernel(f_order, 1, 1, 1, 256, 1, 1, n_groups * 4, st, oargs, nullptr));
                n_order_kernels++;
                S.order = true;             // only now: the kernel that computes it is enqueued
            }
            if (S.order) row_order = T.order;
        }
        if (has_sin) {
            ensure(d_flags, flags_cap, (size_t)n_tiles + 1);                // work list {count, tile, ...} of deferred tiles
            HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(unsigned), st));
        }
        for (uint32_t r0 = 0; r0 < rows_total; r0 += rows_per_grid) {
            uint32_t rows = std::min<uint32_t>(rows_per_grid, rows_total - r0);
            unsigned char *p8 = d8 ? d8 + (size_t)r0 * w * 3 : nullptr;
            double *p64 = d64 ? d64 + (size_t)r0 * w * 3 : nullptr;
            const double *yv = T.yvals + (size_t)r0 * n_yvals;
            unsigned *fl = d_flags;
            unsigned ww = w, yy0 = y0, tile_base = r0 * n_tx, row_base = r0;
            const unsigned long long *gb = gwords;               // indexed by the row of the whole call
            unsigned ntx = n_tx;
            unsigned rpw = 1;                                    // rows per wavefront: a parameter the kernel still has (jit_source.cpp, PIXELS_PROLOGUE)
            const unsigned long long *rwp = T.rwords;            // (maray_jit_pixels_rw and maray_jit_pixels_pp alone have the parameter)
            void *args[] = {&p8, &p64, &yv, &d_tex, &fl, &tile_base, &gb, &ntx, &ww, &yy0, &n_yvals, &tiles, &blk_rows, &blk_stride, &row_base, &yrows, &row_order, &rows, &rpw, &rwp};
            HIP_TRY(hipModuleLaunchKernel(use_pp ? f_pix_pp : use_rw ? f_pix_rw : use_cov ? f_pix_cov : f_pix, gx, rows, 1, 256, 1, 1, 0, st, args, nullptr));
        }
        if (has_sin) slow->render_flagged(w, rb, d8, d64, st, d_flags, T.yvals);   // no-op unless a tile was deferred
    }

    void render_device(uint32_t w, uint32_t, const RowBlocks &rb, void *d8, void *d64, void *stream) override {
        HIP_TRY(hipSetDevice(device));
        launch(w, rb, (unsigned char *)d8, (double *)d64, (hipStream_t)stream, true);
    }

    void render_host_tiles(uint32_t w, uint32_t, const std::vector<RowTile> &tiles, uint32_t row0, uint8_t *rgb8, double *rgb64,
                           const std::function<void(uint32_t, uint32_t)> &done) override {
        HIP_TRY(hipSetDevice(device));
        pipe->run(w, tiles, row0, rgb8, rgb64,
                 [&](const RowBlocks &rb, unsigned char *d8, double *d64, hipStream_t st) { launch(w, rb, d8, d64, st, true); }, done);
    }

    // One shutter picture into d8 (shutter.hpp): frames are ordinary launches on `st`, so the hand-over in launch() orders a
    // call on another stream -- and the scratch with it -- like any other launch.  n = 1 or no parameters: the plain render.
    void launch_shutter(uint32_t w, const RowBlocks &rb, const double *values, uint32_t n, unsigned char *d8, hipStream_t st) {
        const uint32_t np = (uint32_t)param_values.size();
        if (!np || n == 1) {
            if (np) set_params(values, np);
            launch(w, rb, d8, nullptr, st, true);
            return;
        }
        shutter_render(shutter, values, n, np, (size_t)rb.n_rows * w * 3, d8, st,
                       [&](const double *row) { set_params(row, np); },
                       [&](unsigned char *frame) { launch(w, rb, frame, nullptr, st, true); });
    }

    void render_device_shutter(uint32_t w, uint32_t, const RowBlocks &rb, const double *values, uint32_t n, void *d8, void *stream) override {
        HIP_TRY(hipSetDevice(device));
        ShutterRestore<JitBackend> keep{*this, param_values};
        launch_shutter(w, rb, values, n, (unsigned char *)d8, (hipStream_t)stream);
    }

    void render_host_tiles_shutter(uint32_t w, uint32_t, const std::vector<RowTile> &tiles, uint32_t row0, const double *values, uint32_t n,
                                   uint8_t *rgb8, const std::function<void(uint32_t, uint32_t)> &done) override {
        HIP_TRY(hipSetDevice(device));
        ShutterRestore<JitBackend> keep{*this, param_values};
        pipe->run(w, tiles, row0, rgb8, nullptr,
                 [&](const RowBlocks &rb, unsigned char *d8, double *, hipStream_t st) { launch_shutter(w, rb, values, n, d8, st); }, done);
    }

    float time_rows(uint32_t w, uint32_t, const RowBlocks &rb, void *d8, void *d64, int reps) override {
        HIP_TRY(hipSetDevice(device));
        const size_t n = (size_t)rb.n_rows * w * 3;
        unsigned char *p8 = (unsigned char *)d8;
        double *p64 = (double *)d64;
        if (!p8 && !p64) { ensure(d_rgb8, rgb8_cap, n); p8 = d_rgb8; }
        launch(w, rb, p8, p64, own_stream, true);
        launch(w, rb, p8, p64, own_stream, true);          // a geometry's second launch computes its row order
        for (int i = 0; i < 5; i++) launch(w, rb, p8, p64, own_stream, false);      // (the timed launches follow launches of their own kind)
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, own_stream));
        for (int i = 0; i < reps; i++) launch(w, rb, p8, p64, own_stream, false);
        HIP_TRY(hipEventRecord(e1, own_stream));
        HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return ms / (float)(reps > 0 ? reps : 1);
    }

    const char *kernel_name() const override { return ss > 1 ? "maray_jit_pixels_ss" : "maray_jit_pixels"; }
    void launch_counts(uint64_t *row_passes, uint64_t *order_kernels) const override { *row_passes = n_row_passes; *order_kernels = n_order_kernels; }
    uint64_t refine_count() const override { return n_refine_passes; }
    uint64_t census_count() const override { return n_census; }
    uint64_t cover_count() const override { return n_cover; }
    size_t debug_cover_words(uint64_t *words, size_t cap, uint32_t *per_rect) override { return debug_words(words, cap, per_rect, true, true); }
    uint64_t rowscan_count() const override { return n_rowscan; }
    uint64_t prepass_count() const override { return n_prepass; }
    uint64_t deferred_count() override {
        if (!has_sin || !d_flags || !have_last) return 0;
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(hipStreamSynchronize(last_stream));
        unsigned n = 0;
        HIP_TRY(hipMemcpy(&n, d_flags, sizeof n, hipMemcpyDeviceToHost));      // the work list's count: {count, tile, ...}
        return n;
    }
    size_t debug_row_words(uint64_t *xb, size_t xcap, uint64_t *rw, size_t rcap, size_t *n_rwords, uint32_t *per_rect, int *used) override {
        if (!n_gwords || cur_set < 0 || !tabs[cur_set].gbits) throw Error{MARAY_E_ARG, "no guard words: a program without guards, or no launch yet"};
        HIP_TRY(hipSetDevice(device));
        if (have_last) HIP_TRY(hipStreamSynchronize(last_stream));
        *per_rect = n_gwords;
        *used = last_rw ? 1 : 0;
        *n_rwords = 0;
        if (!reuse.sets[cur_set].rowwords || rw_state[cur_set] == COVER_NONE) return 0;
        const size_t n = last_gbits_n, nr = set_rw_n[cur_set];
        if (xb && xcap) HIP_TRY(hipMemcpy(xb, tabs[cur_set].xbits, std::min(n, xcap) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (rw && rcap) HIP_TRY(hipMemcpy(rw, tabs[cur_set].rwords, std::min(nr, rcap) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        *n_rwords = nr;
        return n;
    }
    void debug_row_sets(int *set, uint32_t *kept_sets, uint64_t *kept_bytes, uint64_t *budget, uint64_t *held) const override {
        *set = cur_set;
        *kept_sets = (uint32_t)reuse.kept_sets;
        *kept_bytes = reuse.kept_bytes;
        *budget = reuse.max_bytes;
        uint64_t n = 0;
        for (int s = 1; s < RowReuse::N_SETS; s++) {
            const RowTables &t = tabs[s];
            n += t.yvals_cap * sizeof(double) + t.order_cap * sizeof(unsigned) + t.hits_cap + t.cflags_cap + t.changed_cap +
                 (t.gbits_cap + t.cbits_cap + t.vbits_cap + t.rwords_cap + t.xbits_cap) * sizeof(unsigned long long);
        }
        *held = n;
    }
    size_t debug_guard_words(uint64_t *words, size_t cap, uint32_t *per_rect) override { return debug_words(words, cap, per_rect, false); }
    size_t debug_census_words(uint64_t *words, size_t cap, uint32_t *per_rect) override { return debug_words(words, cap, per_rect, true); }
    // the ROW pass's and the second bounds' words of the set the last launch used, or (census) the words that launch read
    size_t debug_words(uint64_t *words, size_t cap, uint32_t *per_rect, bool census, bool cover = false) {
        if (!n_gwords || cur_set < 0 || !tabs[cur_set].gbits) throw Error{MARAY_E_ARG, "no guard words: a program without guards, or no launch yet"};
        HIP_TRY(hipSetDevice(device));
        if (have_last) HIP_TRY(hipStreamSynchronize(last_stream));
        const size_t n = last_gbits_n;
        const unsigned long long *src = cover && last_cov ? tabs[cur_set].vbits : census && reuse.sets[cur_set].census ? tabs[cur_set].cbits : tabs[cur_set].gbits;
        if (words && cap) HIP_TRY(hipMemcpy(words, src, std::min(n, cap) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        *per_rect = n_gwords;
        return n;
    }
};

}   // namespace

Backend *make_jit_backend(int device, const maray_program &prog, const maray_texture *tex, uint32_t n_tex, uint32_t samples, const maray_refine *refine)
{
    if (hip_device_count() <= 0) throw Error{MARAY_E_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)"};
    auto *b = new JitBackend();
    try {
        b->init(device, prog, tex, n_tex, samples, refine);
    } catch (...) {
        delete b;
        throw;
    }
    return b;
}

}   // namespace maray
