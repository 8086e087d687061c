// jit_source.cpp — tape -> HIP source of the two specialised kernels (product code).  The GPU analogue of the
// reference's wasmer JIT front half:
//
//   jit_source / jit_source_rows   <- wasm::gen_expr / gen_vars / Wasm::from_expr   src/wasm.rs:77-158
//                                     (Expr -> WAT text -> compiled module; one `(local $id f64)` per Let variable)
//
// Differences by design: the input is the lowered tape (one DAG shared by R, G and B, constants folded, Y-only work
// hoisted into a per-row kernel), every op is an inline f64 instruction (the reference's JIT calls host imports for
// abs/recip/step/sin/exp/ln, src/wasm.rs:40-47), max/min follow the interpreter (f64::max/min), not wasm's
// NaN-propagating f64.max/min (src/wasm.rs:58-59).
//
// Generated code: every tape op becomes `const double vN = op(...)`; value slots and ACC disappear (the compiler
// allocates registers), constants become exact hex-float literals or entries of a constant table, y values are scalar
// loads from the row table.  Compiled with -ffp-contract=off so no a*b+c is fused behind the tape's back.
#include "jit_emit.hpp"
#include "row_reuse.hpp"

namespace maray {

// Can the pixel kernel defer tiles to the interpreter?  Only a Sin / Step(Sin) whose argument is not proven bounded can.
bool may_defer_tiles(const maray_program &P)
{
    for (uint32_t i = 0; i < P.n_pix_ops; i++) {
        const uint32_t op = MARAY_INS_OP(P.pix_ops[i]);
        if ((op == MARAY_OP_SIN || op == MARAY_OP_STEPSIN) && !(MARAY_INS_AUX(P.pix_ops[i]) & MARAY_AUX_SIN_BOUNDED)) return true;
    }
    return false;
}

// Every MARAY_JIT_* setting the generators read (each is part of the code key through the text it changes).  Read here and
// nowhere else: a generator takes the struct, so what its text can depend on is what it is handed.
JitKnobs jit_knobs()
{
    JitKnobs K;
    auto off = [](const char *name) { const char *e_ = getenv(name); return e_ && e_[0] == '0'; };
    K.row_guards = !off("MARAY_JIT_ROW_GUARDS");
    if (const char *e_ = getenv("MARAY_JIT_GUARD_W")) K.guard_w = atoi(e_);
    if (const char *e_ = getenv("MARAY_JIT_GUARD_H")) K.guard_h = std::max(0, atoi(e_));        // (set at all: jit_guard_geom keeps the height it is given)
    K.wide_app = !off("MARAY_JIT_WIDE_APP");
    if (const char *e_ = getenv("MARAY_JIT_MIN_REGION")) K.min_region = (uint32_t)atoi(e_);
    K.fuse_cmp = !off("MARAY_JIT_FUSE_CMP");
    K.reduce = !off("MARAY_JIT_REDUCE");
    K.texel_once = !off("MARAY_JIT_TEXEL_ONCE");
    return K;
}

// Which y values are booleans: a dry run of the emitter over the ROW section (its typing is the one the PIXEL section
// will rely on).
std::vector<uint8_t> jit_bool_yvals(const maray_program &P)
{
    std::vector<uint8_t> r(P.n_yvals, 0);
    if (!P.n_row_ops) return r;
    Emitter D(P);
    D.section(P.row_ops, P.n_row_ops, P.n_row_slots, false, "r");
    const uint32_t n_ynum = numeric_yvals(P);
    for (uint32_t k = 0; k < P.n_yvals && k < D.out_is_bool.size() && k < n_ynum; k++) r[k] = D.out_is_bool[k];
    return r;
}

// The guard plan of a program (GuardPlan).  A guard is derived when its source is a MAX tree, boolean-typed all the way
// (on {+0.0, 1.0} max is OR, so "value != 0" distributes over it exactly), whose leaves are sources of other guards.
// Bits are handed out in the order the members are met, so that a group's bits are neighbours (one word, one s_and).
GuardPlan jit_guard_plan(const maray_program &P)
{
    GuardPlan gp;
    const uint32_t n_ynum = numeric_yvals(P), n_guards = P.n_yvals - n_ynum;
    gp.pos.assign(n_guards, -1);
    gp.members.assign(n_guards, {});
    const bool derive = true;
    const RowTapeDeps d = row_tape_deps(P);
    std::vector<int32_t> src(n_guards, -1);                    // op that produces a guard's value
    std::unordered_map<int32_t, uint32_t> guard_of;            // op -> (first) guard it is the source of
    for (uint32_t o : d.outs) {
        const uint32_t aux = MARAY_INS_AUX(P.row_ops[o]);
        if (aux < n_ynum) continue;
        src[aux - n_ynum] = d.deps[o][0];
        if (d.deps[o][0] >= 0) guard_of.emplace(d.deps[o][0], aux - n_ynum);
    }
    std::vector<uint8_t> isb;
    if (derive && P.n_row_ops) {
        Emitter D(P);
        D.section(P.row_ops, P.n_row_ops, P.n_row_slots, false, "r");
        isb = D.is_bool_op;
    }
    // leaves of guard g's MAX tree; false if it is not one
    std::vector<std::vector<uint32_t>> kids(n_guards);
    std::vector<uint8_t> derived(n_guards, 0);
    for (uint32_t g = 0; g < n_guards && derive; g++) {
        const int32_t s0 = src[g];
        if (s0 < 0 || MARAY_INS_OP(P.row_ops[s0]) != MARAY_OP_MAX || !isb[s0]) continue;
        std::vector<int32_t> st = {d.deps[s0][0], d.deps[s0][1]};
        std::vector<uint32_t> leaves;
        bool ok = true;
        while (ok && !st.empty()) {
            const int32_t o = st.back(); st.pop_back();
            if (o < 0) { ok = false; break; }
            auto it = guard_of.find(o);
            if (it != guard_of.end() && it->second != g) { leaves.push_back(it->second); continue; }
            if (MARAY_INS_OP(P.row_ops[o]) == MARAY_OP_MAX && isb[o]) { st.push_back(d.deps[o][1]); st.push_back(d.deps[o][0]); continue; }
            ok = false;
        }
        if (ok && !leaves.empty() && leaves.size() <= 64) { derived[g] = 1; kids[g] = leaves; }
    }
    // bits: members of a derived guard first, in tree order (recursively: a member may be derived itself), then the rest
    std::function<void(uint32_t, std::vector<uint32_t> &)> place = [&](uint32_t g, std::vector<uint32_t> &into) {
        if (derived[g]) {
            if (gp.members[g].empty()) for (uint32_t k : kids[g]) place(k, gp.members[g]);
            into.insert(into.end(), gp.members[g].begin(), gp.members[g].end());
            return;
        }
        if (gp.pos[g] < 0) gp.pos[g] = (int32_t)gp.n_pos++;
        into.push_back((uint32_t)gp.pos[g]);
    };
    std::vector<uint32_t> sink;
    // dearest groups first: their members end up contiguous
    std::vector<uint32_t> order(n_guards);
    for (uint32_t g = 0; g < n_guards; g++) order[g] = g;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return kids[a].size() > kids[b].size(); });
    for (uint32_t g : order) { sink.clear(); place(g, sink); }
    return gp;
}

void jit_guard_layout(const maray_program &P, std::vector<int32_t> &pos, uint32_t *n_words, uint32_t *gw, uint32_t *gh)
{
    const JitKnobs K = jit_knobs();
    const GuardGeom geom = jit_guard_geom(P, K);
    *n_words = jit_guard_words(P, K); *gw = geom.gw; *gh = geom.gh;
    pos = jit_guard_plan(P).pos;
}

// The parameter table of a program with parameters (include/maray_tape.h, SPEC PARAM): a global of every module of the
// program, written by the host alone (JitBackend::send_params finds it by name) and read by scalar loads.  Only sources
// of programs that have parameters contain it; nothing in a source depends on a parameter's VALUE.
static std::string jit_param_table(const maray_program &P)
{
    return "__device__ __attribute__((aligned(64))) double mr_par_tab[" + std::to_string(P.n_params) + "];      // the parameters' values: set by the host between launches\n";
}
// ... behind an address made opaque where the constant table's is: a visible one makes every parameter a loop invariant,
// hoisted out of the tile and pass loops and spilled ("Constants")
static const char PARAM_POINTER[] =
    "    asm volatile(\"\" : \"+s\"(mr_pbase));\n"
    "    const mr_kptr mr_par = (mr_kptr)mr_pbase;\n"
    "    (void)mr_par;\n";

// The ROW section split into chunks that different wavefronts evaluate side by side.  One
// work-item per row is all the parallelism a straight-line ROW kernel has (4096 rows = 64 waves,
// each walking thousands of dependent f64 ops: ~45 us for chess, an eighth of the frame).  The y
// values are independent outputs, so the tape is cut by outputs: chunk k keeps the ops its outputs
// depend on (ops two chunks share are computed in both) and the rest become NOPs.
// Chunk k writes the y values [first[k], first[k] + count[k]): outputs are taken in index order, so that a chunk's
// values are neighbours in a row of the table and leave the kernel as full cache lines (jit_source_rows).
struct RowChunks {
    std::vector<std::vector<uint64_t>> tapes;
    std::vector<uint32_t> first, count;
};
static const uint32_t ROW_CHUNK_MAX_OUTS = 16;      // x 68 x 8 B of LDS per wavefront

RowChunks split_row_tape(const maray_program &P, const RowTapeDeps &d, uint32_t out_limit)
{
    const uint32_t n = P.n_row_ops;
    std::vector<uint32_t> outs;
    for (uint32_t j : d.outs) if (MARAY_INS_AUX(P.row_ops[j]) < out_limit) outs.push_back(j);
    std::sort(outs.begin(), outs.end(), [&](uint32_t x, uint32_t y) { return MARAY_INS_AUX(P.row_ops[x]) < MARAY_INS_AUX(P.row_ops[y]); });
    size_t total = 0;
    (void)row_tape_cone(P, d, outs, &total);
    const size_t per_chunk = 64;
    const uint32_t n_chunks = (uint32_t)std::min<size_t>(64, std::max<size_t>(std::max<size_t>(1, total / per_chunk), (outs.size() + ROW_CHUNK_MAX_OUTS - 1) / ROW_CHUNK_MAX_OUTS));
    const size_t budget = (total + n_chunks - 1) / n_chunks;
    RowChunks rc;
    size_t next = 0;
    while (next < outs.size()) {
        std::vector<uint32_t> mine;
        size_t cost = 0;
        while (next < outs.size() && mine.size() < ROW_CHUNK_MAX_OUTS && cost < budget) {
            // a y value with no OUT of its own between two others would break the chunk's index range: a new chunk starts there
            if (!mine.empty() && MARAY_INS_AUX(P.row_ops[outs[next]]) != MARAY_INS_AUX(P.row_ops[mine.back()]) + 1) break;
            mine.push_back(outs[next++]);
            (void)row_tape_cone(P, d, mine, &cost);
        }
        rc.first.push_back(MARAY_INS_AUX(P.row_ops[mine.front()]));
        rc.count.push_back((uint32_t)mine.size());
        rc.tapes.push_back(row_tape_cone(P, d, mine, &cost));
    }
    if (rc.tapes.empty()) { rc.tapes.emplace_back(n, 0); rc.first.push_back(0); rc.count.push_back(0); }
    return rc;
}

// How the specialised kernels use the row guards of a program: as bits, 64 per word, one set per
// 256-pixel tile of a row (guard_words = 0: not at all -- none, far too many, or switched off).  Up to 12 words a tile's
// words sit in SGPRs; beyond, a guard test reads its word from LDS.
uint32_t jit_guard_words(const maray_program &P, const JitKnobs &K)
{
    if (!K.row_guards || P.n_yvals == numeric_yvals(P)) return 0;
    const uint32_t nw = (jit_guard_plan(P).n_pos + 63) / 64;
    return nw <= 1024 ? std::max(nw, 1u) : 0;       // 1024 words x 8 tiles = 64 KB of LDS
}


// The rectangle a guard is bounded over: `gh` rows x `gw` pixels.  gh = 1 (and gw = 256) when some guard's cone reads Y;
// else every guard bounds its boolean over the rows [YMIN, YMAX] too (include/maray_tape.h) and the rectangle is the
// back-end's choice.  The number of rectangles is what the ROW kernel pays for, their shape is what the PIXEL kernel
// gains from: a shape's edge is met by ~(extent / side + 1) rectangles each way, a wavefront enters regions per 64
// pixels of ONE row, and shapes are tall against 8 rows -- so a rectangle that is narrower and taller by the same factor
// costs the ROW kernel nothing and spares the PIXEL kernel region entries.  Default 64 x 32 (chess @4096^2, frame / board
// crop in us, 256 x 8: 49.3 / 104; 256 x 16: 48.9 / 104; 128 x 16: 45.1 / 92; 64 x 8: 49.0 / 83 -- four times the guard work;
// 64 x 16: 45.5 / 84; 64 x 32: 43.8 / 84; 64 x 64: 45.1 / 86; 64 x 128: 48.1 / 88).  MARAY_JIT_GUARD_W = 64 / 128 / 256,
// MARAY_JIT_GUARD_H = 8 ... 128: measurement knobs.  A strip's words are held one per lane, so a tile's rectangles together
// have to fit a wavefront's 64 lanes: a program with many guard words gets wider rectangles.
GuardGeom jit_guard_geom(const maray_program &P, const JitKnobs &K)
{
    GuardGeom g{256u, 1u};
    const uint32_t nw = jit_guard_words(P, K);
    if (!nw || any_guard_reads_y(P)) return g;
    g.gh = 32u;
    const bool env_h = K.guard_h >= 0;
    if (env_h) { const int v = K.guard_h; if (v == 8 || v == 16 || v == 32 || v == 64 || v == 128) g.gh = (uint32_t)v; }
    uint32_t want = 64u;
    if (K.guard_w == 64 || K.guard_w == 128 || K.guard_w == 256) want = (uint32_t)K.guard_w;
    while (want < 256u && nw * (256u / want) > 64u) want *= 2u;
    if (want == 256u && !env_h) g.gh = 8u;      // wide rectangles gain nothing from height (chess, 256 x 8 / 256 x 32: 48.6 / 50.2 us per frame)
    g.gw = want;
    return g;
}


// Launch order of the PIXEL kernel: groups of rows by what they cost, dearest first, so that the tail of the launch is
// made of cheap blocks.  Cost of a group = set bits in the guard words of its rectangles (shapes that may show there).
// The bits are a function of the program and of the launch's geometry only: the order is computed once per geometry
// (one block; rank by counting) and reused.  Rows of a group stay neighbours (they share guard words and cache lines).
static std::string row_order_kernel(uint32_t n_gwords)
{
    return "extern \"C\" __global__ void __launch_bounds__(256) maray_jit_order(const unsigned long long *__restrict__ gbits, unsigned *__restrict__ order,\n"
         "                                                                  unsigned rows, unsigned n_tx, unsigned yrows)\n{\n"
         "    extern __shared__ unsigned mr_cost[];\n"
         "    const unsigned n_groups = (rows + yrows - 1u) / yrows, n_full = rows / yrows, per = n_tx * " + std::to_string(n_gwords) + "u;\n"
         "    for (unsigned g = threadIdx.x; g < n_groups; g += 256u) {\n"
         "        unsigned c = 0;\n"
         "        for (unsigned i = 0; i < per; i++) c += (unsigned)__builtin_popcountll(gbits[(size_t)g * per + i]);\n"
         "        mr_cost[g] = c;\n"
         "    }\n"
         "    __syncthreads();\n"
         "    for (unsigned g = threadIdx.x; g < n_full; g += 256u) {\n"
         "        const unsigned c = mr_cost[g];\n"
         "        unsigned rank = 0;\n"
         "        for (unsigned h = 0; h < n_full; h++) rank += (mr_cost[h] > c || (mr_cost[h] == c && h < g)) ? 1u : 0u;\n"
         "        for (unsigned i = 0; i < yrows; i++) order[rank * yrows + i] = g * yrows + i;\n"
         "    }\n"
         "    for (unsigned r = n_full * yrows + threadIdx.x; r < rows; r += 256u) order[r] = r;      // a partial last group stays last\n"
         "}\n";
}

// The rectangle of work-item `item` of a guard job, as text: its group of rows and run of pixels, clamped at the ragged
// edges, and the section's XMIN / XMAX / YMIN / YMAX.  Shared by maray_jit_rows' guard jobs and maray_jit_refine: the two
// fill the same table, so they must agree on what a rectangle is.
static std::string guard_rectangle(const GuardGeom &geom)
{
    return   "    const unsigned grp = item / n_tx, tile = item - grp * n_tx;\n"
             "    const unsigned r = grp * yrows, r_last = r + yrows - 1u < rows - 1u ? r + yrows - 1u : rows - 1u;      // launch rows of the group\n"
             "    // (n_tx counts rectangles here; the last 256-pixel tile of a ragged row may own rectangles past the edge: they bound the last pixel)\n"
             "    const unsigned xlo_ = tile * " + std::to_string(geom.gw) + "u, xlo = xlo_ < w - 1u ? xlo_ : w - 1u, xhi = xlo_ + " + std::to_string(geom.gw - 1) + "u < w - 1u ? xlo_ + " + std::to_string(geom.gw - 1) + "u : w - 1u;\n"
             "    // a group never straddles two row blocks (the host picks yrows | blk_rows), so its image rows are consecutive\n"
             "    const double Y = (double)(blk_stride == 0u ? y0 + r : y0 + (r / blk_rows) * blk_stride + r % blk_rows), XMIN = (double)xlo, XMAX = (double)xhi;\n"
             "    const double YMIN = Y, YMAX = Y + (double)(r_last - r);\n";
}

// Source of the ROW kernel, maray_jit_rows: one wavefront per block, blockIdx.y picks the job.
//  y < n_chunks: chunk y of the ROW section, one work-item per row; writes the y values the pixel
//    kernel reads as operands (and, for a program that may defer tiles to the interpreter, the
//    guards too, bounded over the whole row as the interpreter expects).
//  y >= n_chunks: guards 8 (y - n_chunks) .. +7, one work-item per rectangle (group of `yrows` rows,
//    run of jit_guard_geom().gw pixels), evaluated with XMIN / XMAX = the run's ends and YMIN / YMAX = the group's
//    (a bound over a rectangle skips far more than one over the row); writes its byte of
//    the rectangle's guard words (64 guards per word).  yrows = 1 when some guard reads Y.  Small
//    jobs on purpose: each is one long dependent chain, and only more wavefronts hide that.
// One launch for both: the few y-value wavefronts run in the shadow of the guard ones.
// Plain device_math.h: the rare huge-argument tail of sin is a real (out-of-line) call here.
std::string jit_source_rows(const maray_program &P, uint32_t *n_chunks_out, uint32_t *n_gjobs_out)
{
    validate_program(P);
    Emitter E(P);
    const RowTapeDeps deps = row_tape_deps(P);
    const JitKnobs K = jit_knobs();
    const uint32_t n_ynum = numeric_yvals(P), n_gwords = jit_guard_words(P, K);
    const GuardPlan plan = jit_guard_plan(P);
    const GuardGeom geom = jit_guard_geom(P, K);
    // wave-level SKIP ops of the ROW section: a wavefront's lanes are 64 rows, or the 64 rectangles of a band of rows, and
    // agree on the sky only; a job is one wavefront's chain, and every short region it has to test and branch around
    // lengthens it (chess, step minus pixel kernel in us, regions kept from 0 / 12 / 24 / 60 / 200 instructions / none:
    // 7.2 / 6.9 / 6.3 / 6.8 / 8.3 / 8.3)
    E.min_region_row = 24;
    const uint32_t n_gjobs = n_gwords ? (plan.n_pos + 7) / 8 : 0;                // 8 bits = one byte of a word per job
    if (n_gjobs_out) *n_gjobs_out = n_gjobs;
    // the interpreter (which drains deferred tiles from the same y-value table) does read the guard values
    const uint32_t out_limit = may_defer_tiles(P) ? 0xFFFFFFFFu : n_ynum;
    const RowChunks rc = split_row_tape(P, deps, out_limit);
    const std::vector<std::vector<uint64_t>> &chunks = rc.tapes;
    if (n_chunks_out) *n_chunks_out = (uint32_t)chunks.size();
    std::string &s = E.out;
    s += "// generated by libmaray_hip (jit_source.cpp): ROW section, " + std::to_string(P.n_row_ops) + " ops; y values in " +
         std::to_string(chunks.size()) + " chunks, " + std::to_string(P.n_yvals - n_ynum) + " guards in " + std::to_string(n_gwords) + " words,\n"
         "// each bounded over rectangles of " + std::to_string(geom.gw) + " pixels x " + std::to_string(geom.gh) + " rows (the height is a launch parameter, and part of the code key through this line:\n"
         "// a cached code object carries its geometry)\n";
    s += "#include \"device_math.h\"\n\n";
    if (P.n_params) s += jit_param_table(P) + "typedef const __attribute__((address_space(4))) double *mr_kptr;\n";
    // (constants stay literals here: from a table in constant memory like the PIXEL kernel's, the code is a tenth shorter
    // and the kernel 0.8 us slower -- the loads' waits sit in the one chain a job is -- and spills to scratch)
    const unsigned row_block = ROW_BLOCK;
    s += "extern \"C\" __global__ void __launch_bounds__(" + std::to_string(row_block) + ") maray_jit_rows(double *__restrict__ yvals, unsigned long long *__restrict__ gbits,\n"
         "                                                                 const MarayTex *__restrict__ tex,\n"
         "                                                                 unsigned y0, unsigned rows, unsigned n_yvals, unsigned w, unsigned n_tx,\n"
         "                                                                 unsigned blk_rows, unsigned blk_stride, unsigned yrows)\n{\n"
         "    const unsigned item = blockIdx.x * blockDim.x + threadIdx.x;         // (the host keeps the items of a launch below 2^32)\n"
         "    (void)tex; (void)gbits; (void)n_tx;\n" + std::string(P.n_params ? "    unsigned long long mr_pbase = (unsigned long long)mr_par_tab;\n" + std::string(PARAM_POINTER) : "") +
         "    // guard jobs first in the grid (they are the long ones: the y-value jobs fill in behind them): job = the switch index\n"
         "    const unsigned mr_job = blockIdx.y < " + std::to_string(n_gjobs) + "u ? " + std::to_string(chunks.size()) + "u + blockIdx.y : blockIdx.y - " + std::to_string(n_gjobs) + "u;\n"
         "    if (mr_job < " + std::to_string(chunks.size()) + "u) {\n"
         +
         "    // y values: a work-item per row.  A lane's values go to LDS ([value][row], values 68 apart) and leave as rows of the\n"
         "    // table, a chunk's values side by side: full cache lines.  Stored from the registers, a\n"
         "    // wavefront's store touches 64 lines for 8 bytes each -- 1.2 M partial writes per frame, which is what the kernel\n"
         "    // then waits for (11.8 us; the arithmetic needs 2).\n"
         "    __shared__ double mr_ys[" + std::to_string(row_block / 64) + " * " + std::to_string(ROW_CHUNK_MAX_OUTS * 68) + "];\n"
         "    const unsigned mr_lane = threadIdx.x & 63u;\n"
         "    double *ys = mr_ys + (threadIdx.x >> 6) * " + std::to_string(ROW_CHUNK_MAX_OUTS * 68) + "u;\n"
         "    const unsigned row0 = item - mr_lane;                                 // first row of this wavefront\n"
         "    if (row0 >= rows) return;                                            // whole wavefronts only: every lane helps to store\n"
         "    const unsigned r = item;\n"
         "    const double Y = (double)(blk_stride == 0u ? y0 + r : y0 + (r / blk_rows) * blk_stride + r % blk_rows), XMIN = 0.0, XMAX = (double)(w - 1u);\n"
         "    const double YMIN = Y, YMAX = Y;\n"
         "    (void)Y; (void)XMIN; (void)XMAX; (void)YMIN; (void)YMAX; (void)yrows;\n"
         "    unsigned mr_k0 = 0u, mr_kn = 0u;\n"
         "    switch (mr_job) {\n";
    for (size_t k = 0; k < chunks.size(); k++) {
        s += "    case " + std::to_string(k) + ": {\n";
        E.stage_first = (int)rc.first[k];
        E.section(chunks[k].data(), P.n_row_ops, P.n_row_slots, false, "r");
        E.stage_first = -1;
        s += "    mr_k0 = " + std::to_string(rc.first[k]) + "u; mr_kn = " + std::to_string(rc.count[k]) + "u;\n    } break;\n";
    }
    s += "    }\n"
         "    __builtin_amdgcn_wave_barrier();                                       // same wavefront: LDS keeps its order\n"
         "    // lane 16 q + j stores value j of the rows 4 i + q, i = 0 .. 15: an instruction writes four rows of the chunk\n"
         "    const unsigned mr_j = mr_lane & 15u, mr_q = mr_lane >> 4;\n"
         "    double *mr_dst = yvals + (size_t)(row0 + mr_q) * n_yvals + mr_k0 + mr_j;\n"
         "    const size_t mr_step = (size_t)4u * n_yvals;\n"
         "    if (mr_j < mr_kn) {\n"
         "        _Pragma(\"unroll\") for (unsigned i = 0; i < 16u; i++)\n"
         "            if (row0 + 4u * i + mr_q < rows) mr_dst[i * mr_step] = ys[mr_j * 68u + 4u * i + mr_q];\n"
         "    }\n"
         "    return;\n    }\n";
    if (n_gwords) {
        s += "    // guards: (row group, tile), the tiles of a group adjacent\n"
             "    const unsigned n_groups = (rows + yrows - 1u) / yrows;\n"
             "    if (item >= n_groups * n_tx) return;\n"
             + guard_rectangle(geom) +
             "    unsigned long long gacc = 0ull;\n"
             "    double *yout = nullptr;\n"
             "    (void)Y; (void)XMIN; (void)XMAX; (void)YMIN; (void)YMAX; (void)yout;\n"
             "    switch (mr_job - " + std::to_string(chunks.size()) + "u) {\n";
        E.out_guard_bits = true;
        E.guard_first = n_ynum;
        E.plan = &plan;
        for (uint32_t j = 0; j < n_gjobs; j++) {
            std::vector<uint32_t> outs;          // the guards whose bits are 8 j .. 8 j + 7 (derived guards have none: no job computes them)
            for (uint32_t o : deps.outs) {
                const uint32_t aux = MARAY_INS_AUX(P.row_ops[o]);
                if (aux < n_ynum) continue;
                const int32_t k = plan.pos[aux - n_ynum];
                if (k >= (int32_t)(8 * j) && k < (int32_t)(8 * (j + 1))) outs.push_back(o);
            }
            const std::vector<uint64_t> tape = row_tape_cone(P, deps, outs, nullptr);
            s += "    case " + std::to_string(j) + ": {\n";
            E.section(tape.data(), P.n_row_ops, P.n_row_slots, false, "r");
            s += "    } break;\n";
        }
        s += "    }\n"
             "    ((unsigned char *)gbits)[(size_t)item * " + std::to_string(8 * n_gwords) + "u + (mr_job - " + std::to_string(chunks.size()) + "u)] = (unsigned char)gacc;\n";
    }
    s += "}\n";
    if (n_gwords) s += row_order_kernel(n_gwords);
    return s;
}

// Source of maray_jit_refine: the guard half of maray_jit_rows over the program's REFINE section (include/maray_tape.h,
// maray_refine), launched behind it on the same stream.  One work-item per rectangle; blockIdx.y picks a job = one byte
// of the guard words, only the bytes that have a bit with a second bound.  A work-item loads its rectangle's byte; a
// wavefront in which no lane has one of the job's bits set returns at once (chess @4096^2: 93 % of them), the others
// evaluate the job's cones -- a few libm bodies per Step(Sin) factor, which is why this is not part of the ROW section,
// evaluated on every rectangle -- and store byte & (second bounds | bits that have none).  The rectangles, ragged edges
// included, are maray_jit_rows' (guard_rectangle).
std::string jit_source_refine(const maray_program &P, const maray_refine &R, uint32_t *n_jobs_out)
{
    if (n_jobs_out) *n_jobs_out = 0;
    validate_program(P);
    const JitKnobs K = jit_knobs();
    const uint32_t n_gwords = jit_guard_words(P, K);
    if (!R.n_ops || !n_gwords) return "";
    const uint32_t n_ynum = numeric_yvals(P);
    const GuardPlan plan = jit_guard_plan(P);
    const GuardGeom geom = jit_guard_geom(P, K);
    // the section as the ROW section of a program of its own: what the emitter and the cone analysis take
    maray_program Q = P;
    Q.n_consts = R.n_consts; Q.consts = R.consts;
    Q.n_row_ops = R.n_ops; Q.row_ops = R.ops; Q.n_row_slots = R.n_slots;
    const RowTapeDeps deps = row_tape_deps(Q);
    struct Job { uint32_t byte, mask; std::vector<uint32_t> outs; };
    std::vector<Job> jobs;
    for (uint32_t j = 0; j < (plan.n_pos + 7) / 8; j++) {
        Job job{j, 0u, {}};
        for (uint32_t o : deps.outs) {
            const uint32_t aux = MARAY_INS_AUX(R.ops[o]);
            if (aux < n_ynum || aux - n_ynum >= plan.pos.size()) continue;
            const int32_t k = plan.pos[aux - n_ynum];                // (a derived guard has no bit of its own)
            if (k >= (int32_t)(8 * j) && k < (int32_t)(8 * (j + 1))) { job.outs.push_back(o); job.mask |= 1u << (k % 8); }
        }
        if (!job.outs.empty()) jobs.push_back(job);
    }
    if (jobs.empty()) return "";
    if (n_jobs_out) *n_jobs_out = (uint32_t)jobs.size();
    Emitter E(Q);
    std::string &s = E.out;
    s += "// generated by libmaray_hip (jit_source.cpp): REFINE section, " + std::to_string(R.n_ops) + " ops, " + std::to_string(R.n_outs) + " second bounds in " +
         std::to_string(jobs.size()) + " jobs; guards in " + std::to_string(n_gwords) + " words,\n"
         "// each bounded over rectangles of " + std::to_string(geom.gw) + " pixels x " + std::to_string(geom.gh) + " rows\n";
    s += "#include \"device_math.h\"\n\n";
    if (P.n_params) s += jit_param_table(P) + "typedef const __attribute__((address_space(4))) double *mr_kptr;\n";
    s += "extern \"C\" __global__ void __launch_bounds__(" + std::to_string(ROW_BLOCK) + ") maray_jit_refine(unsigned long long *__restrict__ gbits, const MarayTex *__restrict__ tex,\n"
         "                                                                   unsigned y0, unsigned rows, unsigned w, unsigned n_tx,\n"
         "                                                                   unsigned blk_rows, unsigned blk_stride, unsigned yrows)\n{\n"
         "    const unsigned item = blockIdx.x * blockDim.x + threadIdx.x;         // (the host keeps the items of a launch below 2^32)\n"
         "    (void)tex;\n" + std::string(P.n_params ? "    unsigned long long mr_pbase = (unsigned long long)mr_par_tab;\n" + std::string(PARAM_POINTER) : "") +
         "    const unsigned n_groups = (rows + yrows - 1u) / yrows;\n"
         "    const bool mr_in = item < n_groups * n_tx;\n"
         "    // the byte of the rectangle's guard words this job refines, and its bits that have a second bound\n"
         "    unsigned mr_at = 0u, mr_has = 0u;\n"
         "    switch (blockIdx.y) {\n";
    for (size_t j = 0; j < jobs.size(); j++)
        s += "    case " + std::to_string(j) + ": mr_at = " + std::to_string(jobs[j].byte) + "u; mr_has = " + std::to_string(jobs[j].mask) + "u; break;\n";
    s += "    }\n"
         "    unsigned char *mr_p = (unsigned char *)gbits + ((size_t)item * " + std::to_string(8 * n_gwords) + "u + mr_at);\n"
         "    const unsigned mr_b = mr_in ? (unsigned)*mr_p : 0u;\n"
         "    if (mr_ballot((mr_b & mr_has) != 0u) == 0ull) return;                 // no lane of the wavefront has a bit to refine\n"
         + guard_rectangle(geom) +
         "    unsigned long long gacc = 0ull;\n"
         "    (void)Y; (void)XMIN; (void)XMAX; (void)YMIN; (void)YMAX;\n"
         "    switch (blockIdx.y) {\n";
    E.out_guard_bits = true;
    E.guard_first = n_ynum;
    E.plan = &plan;
    for (size_t j = 0; j < jobs.size(); j++) {
        const std::vector<uint64_t> tape = row_tape_cone(Q, deps, jobs[j].outs, nullptr);
        s += "    case " + std::to_string(j) + ": {\n";
        E.section(tape.data(), R.n_ops, R.n_slots, false, "r");
        s += "    } break;\n";
    }
    s += "    }\n"
         "    // a bit stays set unless its second bound is 0; bits without one keep their value\n"
         "    if (mr_in && (mr_b & mr_has) != 0u) *mr_p = (unsigned char)(mr_b & ((unsigned)gacc | ~mr_has));\n"
         "}\n";
    return s;
}

// The general section four pixels per lane: only a short program without guards whose ops are single instructions (no libm
// bodies, no gathers).
bool jit_wide_general(const maray_program &P, uint32_t n_gwords, const JitKnobs &K)        // n_gwords = jit_guard_words(P) (a walk over the ROW tape: the caller has it)
{
    bool heavy = false;
    // texture lookups do not keep a small program from the four-wide form (round 4: four gathers per lane in flight, the scalar
    // unit's share paid once per 256 pixels: config 5 41.5 -> 39.3 us); MARAY_JIT_WIDE_APP=0: one pixel per lane (ablation)
    for (uint32_t i = 0; i < P.n_pix_ops; i++) {
        const uint32_t op = MARAY_INS_OP(P.pix_ops[i]);
        heavy |= op == MARAY_OP_SIN || op == MARAY_OP_EXP || op == MARAY_OP_LN || op == MARAY_OP_STEPSIN || (op == MARAY_OP_APP && !K.wide_app);
    }
    return n_gwords == 0 && !heavy && P.n_pix_slots <= (K.wide_app ? 12u : 6u) && P.n_pix_ops <= 256;
}

// ---- what the PIXEL generators share ---------------------------------------------------------------------------------------
// The set-up of a PIXEL source, the same for every kernel form: the emitter configured for the section, the guard words'
// plan and geometry, the typing of booleans, the reduction plan and the occupancy asked of the compiler.  A generator makes
// one, writes its kernel's text into E.out around E.section(), and ends with splice_constants().
namespace {

struct PixelSetup {
    Emitter E;
    const uint32_t n_ynum, n_gwords;
    const GuardPlan plan;
    const GuardGeom geom;
    const uint32_t sub;                 // guard rectangles per 256-pixel tile (> 1: their words are taken per pass)
    RedPlan reductions;
    int min_waves;
    std::vector<uint8_t> tex_used;      // per image: some App op of the section samples it

    PixelSetup(const maray_program &P, const JitKnobs &K, int min_waves_arg)
        : E(P), n_ynum(numeric_yvals(P)), n_gwords(jit_guard_words(P, K)), plan(jit_guard_plan(P)), geom(jit_guard_geom(P, K)), sub(256u / geom.gw), min_waves(min_waves_arg)
    {
        // Wave-level SKIP ops over fewer than 12 instructions' worth of ops are ignored: a busy tile is bound by the scalar unit
        // (branches, bit tests, mask algebra: 0.59 SALU instructions per cycle and CU against 35 % VALU issue), and a short
        // region's test and branch cost that unit more than its ops cost the vector one (chess board, us per 16.7 Mpx, with
        // guards per 256 x 8 pixels: none ignored 111, 24: 104; with guards per 64 x 32: 8 / 12 / 16 ... 32 / 64 / 200:
        // 83.3 / 82.4 / 84.7 / 85.4 / 128).
        // (round 4: 24, from 12; pixel kernel / step / board 27.34 / 34.02 / 60.9 against 27.6 / 34.2-34.4 / 61.2 us, the same sign in round 3's table)
        E.min_region = K.min_region;
        E.ybool = jit_bool_yvals(P);
        E.fuse_cmp = K.fuse_cmp;
        E.ktab = true;
        for (uint32_t i = 0; i < P.n_pix_ops && E.sin_k < 0; i++)
            if (MARAY_INS_OP(P.pix_ops[i]) == MARAY_OP_STEPSIN) {
                // the first cache line of the table: what every leaf with a texture reads
                static const double sin_k[8] = {0x1.45f306dc9c883p-1, 0x1.8p52, 0x1.921fb58000000p+0, -0x1.dde973c000000p-27, -0x1.cb3b398000000p-55, -0x1.d747f23e32ed7p-83, 0x1p-70, 0.0};
                E.sin_k = 0;
                E.ktab_vals.assign(sin_k, sin_k + 8);
            }
        E.ignore_row_guards = n_gwords == 0;
        if (n_gwords) { E.guard_first = n_ynum; E.guard_words = n_gwords; E.plan = &plan; E.gw_inline_max = GW_INLINE_MAX; }
        if (!E.ignore_row_guards) {         // dry run: which ops yield lane masks
            Emitter D(P);
            D.ignore_row_guards = true;
            D.min_region = E.min_region;
            D.ybool = E.ybool;
            D.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
            E.bool_hint = D.is_bool_op;
            // OR trees of guarded shapes: evaluated from their set guard bits (RedPlan).  MARAY_JIT_REDUCE=0: walked as written (ablation)
            if (K.reduce) reductions = plan_reductions(P.pix_ops, P.n_pix_ops, P.n_pix_slots, D.is_bool_op, n_ynum, plan, E.ybool);
        }
        // Occupancy asked of the compiler.  Walking a tree of bit tests needs the SGPRs of 6 waves per SIMD (up to 102; at 8 the
        // compiler gets 76-80 and spilled ~400 of them to VGPR lanes, in the skeleton of bit tests and branches every pass walked;
        // chess needs 38 VGPRs either way); with the tree evaluated as a reduction chess fits 78 and runs 8 (frame 29.9 -> 29.5 us,
        // sky 12.3 -> 11.5, board 67.1 -> 65.1)
        if (min_waves_arg == 0) min_waves = reductions.empty() ? 6 : 8;
        for (uint32_t i = 0; i < P.n_pix_ops; i++)
            if (MARAY_INS_OP(P.pix_ops[i]) == MARAY_OP_APP) { const uint32_t img = MARAY_INS_AUX(P.pix_ops[i]) / 5u; if (tex_used.size() <= img) tex_used.resize(img + 1, 0); tex_used[img] = 1; }
        E.texel_once = !tex_used.empty() && K.texel_once;       // MARAY_JIT_TEXEL_ONCE=0: a call of mr_app per App op (= round 3; ablation)
    }
    PixelSetup(const PixelSetup &) = delete;        // (E.plan points into this object)

    // the descriptors of the textures the section samples: scalar loads, once per wavefront
    std::string texture_loads() const
    {
        std::string s;
        for (size_t img = 0; img < tex_used.size() && E.texel_once; img++)
            if (tex_used[img]) s += "    const MarayTex mr_t" + std::to_string(img) + " = tex[" + std::to_string(img) + "];\n";
        return s;
    }

    // Ends a source: E.out's three markers become what the section turned out to need.  /*MR_KTAB*/: `device_text` (functions
    // of the kernel form that use the types above the marker) and the constant table; /*MR_KBASE*/: the table's address,
    // taken once per tile; /*MR_KC*/: that address made opaque once per pass (see PASS_TABLES).
    std::string splice_constants(const std::string &device_text)
    {
        std::string &s = E.out;
        std::string tab = device_text;
        if (E.P.n_params) tab += jit_param_table(E.P);
        if (!E.ktab_vals.empty()) {
            tab += "__constant__ __attribute__((aligned(64))) double mr_kc_tab[" + std::to_string(E.ktab_vals.size()) + "] = {";
            for (size_t j = 0; j < E.ktab_vals.size(); j++) { tab += (j % 6 ? " " : "\n    "); tab += lit(E.ktab_vals[j]); tab += ","; }
            tab += "\n};\n";
        }
        s.replace(s.find("/*MR_KTAB*/"), 11, tab);
        for (size_t at; (at = s.find("/*MR_KBASE*/")) != std::string::npos;)
            s.replace(at, 12, std::string(E.ktab_vals.empty() ? "" : "    unsigned long long mr_kbase = (unsigned long long)mr_kc_tab;\n") +
                              (E.P.n_params ? "    unsigned long long mr_pbase = (unsigned long long)mr_par_tab;\n" : ""));
        const std::string kc = std::string(E.ktab_vals.empty() ? "    asm volatile(\"\" ::: \"memory\");\n" :
                                           "    asm volatile(\"\" : \"+s\"(mr_kbase) :: \"memory\");\n"
                                           "    const mr_kptr mr_kc = (mr_kptr)mr_kbase;\n") + (E.P.n_params ? PARAM_POINTER : "");
        for (size_t at; (at = s.find("/*MR_KC*/")) != std::string::npos;) s.replace(at, 9, kc);
        return s;
    }
};

}   // namespace

// What opens a pass of any width: the y values and the constant table behind addresses made opaque (LICM would hoist every
// constant and y value out of the loops and spill them).  `mr_ybase` is declared by the kernel form in front of this.
static const char PASS_TABLES[] =
    "    asm volatile(\"\" : \"+s\"(mr_ybase));\n"
    "    mr_kptr yv = (mr_kptr)mr_ybase;\n"
    "    const __attribute__((address_space(4))) unsigned *yw = (const __attribute__((address_space(4))) unsigned *)yv;\n"
    "    (void)yv; (void)yw;\n/*MR_KC*/";

// ---- maray_jit_pixels: the pieces of its text ---------------------------------------------------------------------------------
// The kernel once took two rows per wavefront in its busy tiles (measured, lost, removed).  The `rows` and
// `rpw` parameters, the two comment lines about rpw = 2 in PIXELS_HEAD and the "(of both rows)" in PIXELS_PROLOGUE's mr_tp
// comment are what is left of it in the emitted text: the host passes rpw = 1, and they go with the next change that is
// meant to change these kernels (and measures them), not with one that must keep their text.
static const char PIXELS_PROLOGUE[] =
    "#define MR_VEC4 1\n"
    "__shared__ unsigned mr_slow[4];           // per wavefront: some Sin of the tile at hand needs the slow path\n"
    "__shared__ unsigned mr_tp[4 * 256];       // per wavefront: the packed pixels of a tile's four passes (of both rows)\n"
    "__device__ inline double mr_defer_sin(double) { ((volatile unsigned *)mr_slow)[threadIdx.x >> 6] = 1u; return 0.0; }\n"
    "#define MR_SIN_HUGE(x) mr_defer_sin(x)   // plain Sin ops: flag the tile from the (rare) branch\n"
    "#include \"device_math.h\"\n"
    "typedef const __attribute__((address_space(4))) double *mr_kptr;\n"
    "struct __attribute__((aligned(4))) mr_u3 { unsigned a, b, c; };\n"
    "struct __attribute__((aligned(16))) mr_u4 { unsigned a, b, c, d; };\n"
    "__device__ inline mr_mask mr_lane64(unsigned long long v, unsigned lane)      // lane `lane` (wave-uniform) of a per-lane 64-bit value -> SGPR pair\n"
    "{\n"
    "    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)lane);\n"
    "    return ((mr_mask)hi << 32) | lo;\n"
    "}\n/*MR_KTAB*/\n";

// one 64-pixel run: f64 planes (24 B per lane) and / or RGB8 (48 lanes assemble a dword each from two neighbours'
// packed colours; ragged ends and unaligned rows store bytes)
static const char MR_STORE_RUN[] =
    "__device__ inline void mr_store_run(unsigned char *__restrict__ rgb8, double *__restrict__ rgb64, size_t row_px, unsigned xw, unsigned w,\n"
    "                                    unsigned lane, unsigned src, unsigned shift, unsigned pk, double c0, double c1, double c2)\n{\n"
    "    const unsigned x = xw + lane;\n"
    "    if (rgb64 && x < w) { const size_t p = (row_px + x) * 3; rgb64[p] = c0; rgb64[p + 1] = c1; rgb64[p + 2] = c2; }\n"
    "    if (rgb8) {\n"
    "        unsigned char *wave_out = rgb8 + (row_px + xw) * 3;\n"
    "        if (xw + 64u <= w && ((size_t)wave_out & 3u) == 0u) {                // wave-uniform\n"
    "            const unsigned pa = (unsigned)__builtin_amdgcn_ds_bpermute((int)(src * 4u), (int)pk);\n"
    "            const unsigned pb = (unsigned)__builtin_amdgcn_ds_bpermute((int)(src * 4u + 4u), (int)pk);\n"
    "            const unsigned dw = (unsigned)((((unsigned long long)pb << 24) | pa) >> shift);\n"
    "            if (lane < 48u) ((unsigned *)wave_out)[lane] = dw;\n"
    "        } else if (x < w) {\n"
    "            unsigned char *q = rgb8 + (row_px + x) * 3;\n"
    "            q[0] = (unsigned char)pk; q[1] = (unsigned char)(pk >> 8); q[2] = (unsigned char)(pk >> 16);\n"
    "        }\n"
    "    }\n"
    "}\n";

// the kernel's parameters and what a wavefront works out once: its strip, its row, the row's y values and Y
static std::string pixels_head(int min_waves)
{
    return "extern \"C\" __global__ void __launch_bounds__(256, " + std::to_string(min_waves) +
         ") maray_jit_pixels(unsigned char *__restrict__ rgb8, double *__restrict__ rgb64,\n"
         "                                                                    const double *__restrict__ yvals, const MarayTex *__restrict__ tex,\n"
         "                                                                    unsigned *__restrict__ tile_list, unsigned tile_base,\n"
         "                                                                    const unsigned long long *__restrict__ gbits, unsigned n_tx,\n"
         "                                                                    unsigned w, unsigned y0, unsigned n_yvals, unsigned tiles,\n"
         "                                                                    unsigned blk_rows, unsigned blk_stride, unsigned row_base, unsigned yrows,\n"
         "                                                                    const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw)\n{\n"
         "    const unsigned mr_wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), mr_lane = threadIdx.x & 63u;\n"
         "    // (workgroups go to the 8 XCDs round robin by their linear id: with 2, 4 or 8 blocks per row a column of the image\n"
         "    // always meets the same XCDs; rotating a row's strips by the row was measured and is not worth it, DESIGN.md 7.1)\n"
         "    const unsigned tile0 = (blockIdx.x * 4u + mr_wv) * tiles;               // this wavefront's strip of the row\n"
         "    if (tile0 >= n_tx) return;\n"
         "    // rows of this launch (dearest groups of rows first); row_base + r = row of the whole call.  rpw = 2 (two-row kernels, when the\n"
         "    // launch's guard groups have an even number of rows): this wavefront owns rows r and r + 1 of one group\n"
         "    const unsigned mr_rr = blockIdx.y * rpw;\n"
         "    const unsigned r = row_order ? row_order[mr_rr] : mr_rr;\n"
         "    (void)rows;\n"
         "    const unsigned long long mr_ybase0 = (unsigned long long)(yvals + (size_t)r * n_yvals);\n"
         "    // -> image row (RowBlocks); one range of rows (blk_stride == 0) needs no division, and yrows is a power of two\n"
         "    const double Y = (double)(blk_stride == 0u ? y0 + row_base + r : y0 + ((row_base + r) / blk_rows) * blk_stride + (row_base + r) % blk_rows);\n"
         "    (void)Y; (void)tex; (void)gbits; (void)yrows; (void)tile_list; (void)tile_base;\n";
}

// How the guard words of the tile or pass at hand reach the section's bit tests -- four ways, by how many words a rectangle
// has (n_gwords; 0: the program has no guards) and how many rectangles a tile (sub):
//   in_sgprs (<= GW_INLINE_MAX words): a strip's words arrive with one vector load per wavefront (lane i holds word i, mr_gv)
//     and each word of the rectangle at hand is named, gq<j>, taken with v_readlane per tile (sub == 1) or per pass (sub > 1)
//     -- one memory latency per strip instead of one per tile;
//   else one word per lane, loaded per tile: mr_gt0 holds the words of the tile's rectangles (sub > 1: <= 64 together,
//     jit_guard_geom), or mr_gt<j> the words 64 j .. 64 j + 63 of its one rectangle; a test takes its word with v_readlane.
namespace {
struct GuardWords {
    uint32_t n, sub;
    bool in_sgprs;
    std::string nw, tw, esub;       // as text: words per rectangle, words per tile, the rectangle of pass e inside its tile
    GuardWords(uint32_t n_gwords, uint32_t sub_)
        : n(n_gwords), sub(sub_), in_sgprs(n_gwords && n_gwords <= GW_INLINE_MAX), nw(std::to_string(n_gwords)), tw(std::to_string(sub_ * n_gwords)),
          esub("(e >> " + std::to_string(sub_ == 4 ? 0 : 1) + "u)") {}
    bool per_lane() const { return n && !in_sgprs; }
    uint32_t lane_vars() const { return (n + 63) / 64; }       // mr_gt<j> of a tile with one rectangle
};
}   // namespace

// once per strip: where its guard words are, and (in_sgprs) the words themselves
static std::string strip_guard_fetch(const GuardWords &g)
{
    std::string s;
    if (g.n)
        s += "    const unsigned long long mr_gbase0 = (unsigned long long)(gbits + ((size_t)((row_base + r) >> __builtin_ctz(yrows)) * n_tx + tile0) * " + g.tw + "u);\n";
    if (g.in_sgprs)
        s += "    const unsigned mr_gn = (n_tx - tile0 < tiles ? n_tx - tile0 : tiles) * " + g.tw + "u;       // <= 64: the host bounds `tiles`\n"
             "    const unsigned long long mr_gv = mr_lane < mr_gn ? ((const unsigned long long *)mr_gbase0)[mr_lane] : 0ull;\n" +
             (g.sub > 1 ? "    const unsigned long long mr_gnz = mr_ballot(mr_gv != 0ull);            // which of the strip's words have a bit set\n" : "");
    return s;
}

// once per tile: its words, one per lane (per_lane) or named (in_sgprs, one rectangle per tile)
static std::string tile_guard_fetch(const GuardWords &g)
{
    std::string s;
    if (g.per_lane()) {
        s += "    unsigned long long mr_gbase = mr_gbase0;\n"
             "    asm volatile(\"\" : \"+s\"(mr_gbase));\n";
        if (g.sub > 1)
            s += "    unsigned long long mr_gt0 = mr_lane < " + g.tw + "u ? ((const unsigned long long *)mr_gbase)[t * " + g.tw + "u + mr_lane] : 0ull;\n";
        else
            for (uint32_t j = 0; j < g.lane_vars(); j++)
                s += "    unsigned long long mr_gt" + std::to_string(j) + " = " + std::to_string(64 * j) + "u + mr_lane < " + g.nw + "u ? ((const unsigned long long *)mr_gbase)[t * " + g.nw + "u + " +
                     std::to_string(64 * j) + "u + mr_lane] : 0ull;\n";
    } else if (g.in_sgprs && g.sub == 1)
        for (uint32_t j = 0; j < g.n; j++)
            s += "    mr_mask gq" + std::to_string(j) + " = mr_lane64(mr_gv, t * " + g.nw + "u + " + std::to_string(j) + "u);\n";
    return s;
}

// once per pass: the guard words of the rectangle at hand, opaque anew in every pass: left visible, all their bit tests are
// loop invariants too (168 booleans for chess, hoisted and spilled to VGPR lanes)
static std::string pass_guard_words(const GuardWords &g)
{
    std::string s;
    if (g.per_lane() && g.sub > 1)
        s = "    asm volatile(\"\" : \"+v\"(mr_gt0));\n"
            "    const unsigned mr_gsub = " + g.esub + " * " + g.nw + "u;           // first word of this pass's rectangle\n"
            "    const unsigned long long mr_gnzp = mr_ballot(mr_gt0 != 0ull) >> mr_gsub;      // which of its words have a bit set\n"
            "    (void)mr_gnzp;\n";
    else if (g.in_sgprs && g.sub > 1)
        for (uint32_t j = 0; j < g.n; j++) {
            const std::string k = std::to_string(j);
            s += "    mr_mask gq" + k + " = mr_lane64(mr_gv, (t * " + std::to_string(g.sub) + "u + " + g.esub + ") * " + g.nw + "u + " + k + "u);\n"
                 "    asm volatile(\"\" : \"+s\"(gq" + k + "));\n";
        }
    else if (g.in_sgprs)
        for (uint32_t j = 0; j < g.n; j++) s += "    asm volatile(\"\" : \"+s\"(gq" + std::to_string(j) + "));\n";
    else
        for (uint32_t j = 0; j < g.lane_vars(); j++) {
            const std::string k = std::to_string(j);
            s += "    asm volatile(\"\" : \"+v\"(mr_gt" + k + "));\n"
                 "    const unsigned long long mr_gnz" + k + " = mr_ballot(mr_gt" + k + " != 0ull);      // which of the tile's words have a bit set\n"
                 "    (void)mr_gnz" + k + ";\n";
        }
    return s;
}

// `if (no guard bit of this tile is set) {`: what sends a tile to the wide variant
static std::string sky_test(const GuardWords &g)
{
    if (g.per_lane() && g.sub > 1) return "    if (mr_ballot(mr_gt0 != 0ull) == 0ull) {\n";
    if (g.sub > 1) return "    if (((mr_gnz >> (t * " + g.tw + "u)) & " + std::to_string((1ull << (g.sub * g.n)) - 1ull) + "ull) == 0ull) {\n";
    std::string any = g.in_sgprs ? "gq0" : "mr_gt0";
    for (uint32_t j = 1; j < (g.in_sgprs ? g.n : g.lane_vars()); j++) any += (g.in_sgprs ? " | gq" : " | mr_gt") + std::to_string(j);
    return g.in_sgprs ? "    if ((" + any + ") == 0ull) {\n" : "    if (mr_ballot((" + any + ") != 0ull) == 0ull) {\n";
}

// the y-value table of a pass of maray_jit_pixels (its one row's) and PASS_TABLES
static const std::string PIXELS_PASS_TABLES = std::string("    unsigned long long mr_ybase = mr_ybase0;\n") + PASS_TABLES;

// after a pass's section: has some Sin of it sent the tile to the interpreter?
static std::string defer_pass(bool defer)
{
    return defer ? "    mr_slow_tile |= mr_ballot(mr_defer != 0.0f) != 0ull || ((volatile unsigned *)mr_slow)[mr_wv] != 0u;      // wave-uniform\n" : "";
}

// WIDE: a whole tile in one pass, four pixels per lane.  Opens the block the section goes into ...
static std::string wide_open(const GuardWords &g)
{
    return "    {\n" + PIXELS_PASS_TABLES + (g.sub > 1 ? std::string() : pass_guard_words(g)) +
        "    const unsigned xa = x0 + mr_xl;                                        // this lane's first pixel\n"
        "    const mr_d X((double)xa, (double)(xa + mr_xs), (double)(xa + 2u * mr_xs), (double)(xa + 3u * mr_xs));\n"
        "    mr_d o0 = 0.0, o1 = 0.0, o2 = 0.0;\n"
        "    float mr_defer = 0.0f;                     // fused Step(Sin) ops count their undecided cases in here\n"
        "    (void)X; (void)mr_defer;\n";
}

// ... and packs, stores and closes it: a lane's four RGB8 pixels are 12 contiguous bytes; with f64 planes, four 64-pixel runs
static std::string wide_close(bool defer)
{
    return defer_pass(defer) +
        "    const unsigned p0 = mr_cast_u8(o0.a) | (mr_cast_u8(o1.a) << 8) | (mr_cast_u8(o2.a) << 16);\n"
        "    const unsigned p1 = mr_cast_u8(o0.b) | (mr_cast_u8(o1.b) << 8) | (mr_cast_u8(o2.b) << 16);\n"
        "    const unsigned p2 = mr_cast_u8(o0.c) | (mr_cast_u8(o1.c) << 8) | (mr_cast_u8(o2.c) << 16);\n"
        "    const unsigned p3 = mr_cast_u8(o0.d) | (mr_cast_u8(o1.d) << 8) | (mr_cast_u8(o2.d) << 16);\n"
        "    if (mr_wide) {\n"
        "        if (rgb8) {\n"
        "            unsigned char *q = rgb8 + (row_px + xa) * 3;                      // this lane's 12 bytes\n"
        "            if (x0 + 256u <= w && ((size_t)(rgb8 + (row_px + x0) * 3) & 3u) == 0u) {     // wave-uniform: a whole tile whose bytes start on a dword\n"
        "                mr_u3 d;\n"
        "                d.a = p0 | (p1 << 24); d.b = (p1 >> 8) | (p2 << 16); d.c = (p2 >> 16) | (p3 << 8);\n"
        "                *(mr_u3 *)q = d;\n"
        "            } else {\n"
        "                const unsigned pk[4] = {p0, p1, p2, p3};\n"
        "                for (unsigned e = 0; e < 4u; e++)\n"
        "                    if (xa + e < w) { q[3 * e] = (unsigned char)pk[e]; q[3 * e + 1] = (unsigned char)(pk[e] >> 8); q[3 * e + 2] = (unsigned char)(pk[e] >> 16); }\n"
        "            }\n"
        "        }\n"
        "    } else {\n"
        "        const unsigned pk[4] = {p0, p1, p2, p3};\n"
        "        const double c0[4] = {o0.a, o0.b, o0.c, o0.d}, c1[4] = {o1.a, o1.b, o1.c, o1.d}, c2[4] = {o2.a, o2.b, o2.c, o2.d};\n"
        "        _Pragma(\"unroll\") for (unsigned e = 0; e < 4u; e++)\n"
        "            mr_store_run(rgb8, rgb64, row_px, x0 + 64u * e, w, mr_lane, mr_src, mr_shift, pk[e], c0[e], c1[e], c2[e]);\n"
        "    }\n"
        "    }\n";
}

// NARROW: one wavefront, four passes of 64 pixels (a loop, not unrolled).  Opens the loop the section goes into ...
static std::string narrow_open(const GuardWords &g)
{
    return "    const bool mr_fast = rgb8 && x0 + 256u <= w && ((size_t)(rgb8 + (row_px + x0) * 3) & 3u) == 0u;      // wave-uniform\n"
           "    _Pragma(\"unroll 1\") for (unsigned e = 0; e < 4u; e++) {\n" + PIXELS_PASS_TABLES + pass_guard_words(g) +
           "    const unsigned xw = x0 + 64u * e, x = xw + mr_lane;\n"
           "    const double X = (double)x;\n"
           "    double o0 = 0.0, o1 = 0.0, o2 = 0.0;\n"
           "    float mr_defer = 0.0f;\n"
           "    (void)X; (void)mr_defer;\n";
}

// ... and closes it: the passes leave their packed pixels in LDS (same-wave traffic: no barrier) and a whole aligned tile is
// stored as a dwordx3 per lane
static std::string narrow_close(bool defer)
{
    return defer_pass(defer) +
           "    const unsigned pk = mr_cast_u8(o0) | (mr_cast_u8(o1) << 8) | (mr_cast_u8(o2) << 16);\n"
           "    if (mr_fast) {\n"
           "        mr_tp[mr_wv * 256u + 64u * e + mr_lane] = pk;\n"
           "        mr_store_run(nullptr, rgb64, row_px, xw, w, mr_lane, mr_src, mr_shift, pk, o0, o1, o2);\n"
           "    } else mr_store_run(rgb8, rgb64, row_px, xw, w, mr_lane, mr_src, mr_shift, pk, o0, o1, o2);\n"
           "    }\n"
           "    if (mr_fast) {\n"
           "        __builtin_amdgcn_wave_barrier();                                     // same wavefront wrote them: LDS keeps its order\n"
           "        const mr_u4 p = *(const mr_u4 *)&mr_tp[mr_wv * 256u + 4u * mr_lane];\n"
           "        mr_u3 d;\n"
           "        d.a = p.a | (p.b << 24); d.b = (p.b >> 8) | (p.c << 16); d.c = (p.c >> 16) | (p.d << 8);\n"
           "        *(mr_u3 *)(rgb8 + (row_px + x0 + 4u * mr_lane) * 3) = d;\n"
           "        __builtin_amdgcn_wave_barrier();\n"
           "    }\n";
}

// closes a tile: the work list entry of a tile some Sin of which needs the slow path
static std::string tile_end(bool defer)
{
    return defer ? "    if (mr_slow_tile && mr_lane == 0u) tile_list[1u + atomicAdd(&tile_list[0], 1u)] = tile_base + r * n_tx + tile0 + t;\n" : "";
}

// Source of the PIXEL kernel, maray_jit_pixels.  A wavefront owns a strip of `tiles` consecutive 256-pixel tiles of one
// row (blockIdx.y); a block is four wavefronts = four neighbouring strips that share nothing but the instruction cache:
// no staging, no barrier.  The strip's guard words arrive with one vector load (lane i = word i); per tile one scalar
// test of a ballot picks the variant:
//
//  * WIDE, four pixels per lane (device_math.h, MR_VEC4: every value four f64, every boolean four lane masks).  The
//    variant of a tile none of whose guard bits is set (every guarded region is the literal 0: for chess the background,
//    one multiply), and the whole section of a small program without guards (config 2: six ops).  The scalar unit's
//    share of a tile and the store's address arithmetic are paid once per 256 pixels, and a lane's four RGB8 pixels are
//    12 contiguous bytes: one global_store_dwordx3, no cross-lane packing.  This is the path that is bound by the store
//    (3 B per pixel) and little else.
//  * NARROW, one pixel per lane, four passes of 64 pixels (a loop: the section's code exists once).  The variant of a
//    tile where shapes may show.  Regions are entered per 64 pixels, where a wave-level SKIP op still finds all lanes
//    agreeing; values are single f64.  The passes leave their packed pixels in LDS (same-wave traffic: no barrier) and
//    the tile is stored like a wide one.
//
// When f64 planes are wanted too, element e of a wide lane l is pixel x0 + 64 e + l and every 64-pixel run is stored on
// its own (24 B per lane, the coalesced pattern of the f64 planes).  A Sin whose argument is huge (|x| >= 105414350), inf
// or NaN does not call the slow reduction here (a call site per Sin op would force every live value through scratch): the
// tile is flagged instead and re-evaluated by the tape interpreter kernel afterwards, so the final raster is identical.
// Layouts that were measured and lost (a wavefront per 64 pixels with guard words staged in LDS, a busy tile on the
// block's four wavefronts side by side, persistent wavefronts, two pixels per lane, two rows per wavefront, guard words by
// scalar loads, a sky loop of its own ...) are history: DESIGN.md section 7.1, profiles/r2_ablations.jsonl.
// the kernel itself, from `head` (its name and parameters) to its closing brace, into S.E.out: maray_jit_pixels, and with the
// emitter's use_cover flag set maray_jit_pixels_cov (jit_source_cover)
// (strip_fetch: the strip's guard fetch where it is not strip_guard_fetch()'s -- maray_jit_pixels_rw, jit_source_rowwords)
// (pp: the wide pre-pass of a busy tile's leafless rectangles -- maray_jit_pixels_pp, jit_source_prepass; everything it adds
// to the text stands between PP_OPEN and PP_CLOSE)
namespace {
struct PrepassPlan { std::vector<std::pair<uint32_t, uint32_t>> roots; };       // (root op of a boolean reduction, its cover bit in the last guard word)
const char PP_OPEN[] = "    /*mr_pp{*/\n", PP_CLOSE[] = "    /*mr_pp}*/\n";
}   // namespace
static std::string prepass_tile(PixelSetup &S, const maray_program &P, const GuardWords &g, const PrepassPlan &pp, bool defer);

static void pixels_kernel(PixelSetup &S, const maray_program &P, const JitKnobs &K, const std::string &head, const std::string *strip_fetch = nullptr,
                          const PrepassPlan *pp = nullptr)
{
    Emitter &E = S.E;
    const GuardWords g(S.n_gwords, S.sub);
    const bool defer = may_defer_tiles(P), wide_general = jit_wide_general(P, S.n_gwords, K);
    if (g.per_lane() && g.sub > 1) E.gw_lane_base = "mr_gsub";
    auto section = [&](const char *td, const char *tm, bool sky, const RedPlan *rplan) {
        E.td = td; E.tm = tm; E.assume_guards_zero = sky; E.rplan = rplan;
        E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
    };
    std::string &s = E.out;
    s += head + S.texture_loads() + (strip_fetch ? *strip_fetch : strip_guard_fetch(g)) +
         "    const bool mr_wide = rgb64 == nullptr;                                   // wide variants: element e of lane l is pixel x0 + 4 l + e, else x0 + 64 e + l\n"
         "    const unsigned mr_xl = mr_wide ? 4u * mr_lane : mr_lane, mr_xs = mr_wide ? 1u : 64u;\n"
         "    const unsigned mr_src = (mr_lane * 4u) / 3u, mr_shift = ((mr_lane * 4u) % 3u) * 8u;   // RGB8 packing of one 64-pixel run\n"
         "    const size_t row_px = (size_t)r * w;\n"
         "    for (unsigned t = 0; t < tiles; t++) {\n"
         "    const unsigned x0 = (tile0 + t) * 256u;\n"
         "    if (x0 >= w) break;\n"
         "    // y values, constants, guard words: scalar loads where they are used, from addresses made opaque in every trip (fresh\n"
         "    // copies: an asm output carried around the loop counts as divergent once a lane-dependent branch sits in the loop)\n"
         "/*MR_KBASE*/" + tile_guard_fetch(g);
    if (defer) s += "    ((volatile unsigned *)mr_slow)[mr_wv] = 0u;\n    bool mr_slow_tile = false;\n";
    if (g.n) {          // the variant of a tile with no guard bit set, four pixels per lane
        s += sky_test(g) + wide_open(g);
        section("mr_d", "mr_m", true, nullptr);
        s += wide_close(defer) + tile_end(defer) + "    continue;\n    }\n";
    }
    if (wide_general) {
        s += wide_open(g);
        section("mr_d", "mr_m", false, nullptr);
        s += wide_close(defer) + tile_end(defer);
    } else if (pp) {
        // narrow_open()'s text with the pre-pass behind its first line (mr_fast) and the skip of the leafless passes at the head
        // of its loop.  The pre-pass's section is emitted AFTER the narrow one and put in front of it: the narrow section's
        // label numbers are then maray_jit_pixels_rw's
        const std::string open = narrow_open(g);
        const size_t nl = open.find('\n'), lp = open.find("e++) {\n");
        if (nl == std::string::npos || lp == std::string::npos || lp < nl) throw Error{MARAY_E_INTERNAL, "the narrow loop's text is not what the pre-pass is spliced into"};
        const size_t line1 = nl + 1, loop = lp + 7;
        s += open.substr(0, line1);
        const size_t at = s.size();
        s += open.substr(line1, loop - line1) + PP_OPEN + "    if (((mr_ppleafy >> e) & 1u) == 0u) continue;      // its pixels are the pre-pass's\n" + PP_CLOSE + open.substr(loop);
        section("double", "mr_mask", false, &S.reductions);
        s += narrow_close(defer) + tile_end(defer);
        std::string rest;
        rest.swap(s);
        const std::string tile = prepass_tile(S, P, g, *pp, defer);      // (appends its section to s, which is E.out)
        s = rest;
        s.insert(at, tile);
    } else {
        s += narrow_open(g);
        section("double", "mr_mask", false, &S.reductions);
        s += narrow_close(defer) + tile_end(defer);
    }
    s += "    }\n}\n";
}

// The pre-pass of a tile of maray_jit_pixels_pp, between narrow_open()'s mr_fast and its loop: which of the tile's four
// rectangles are leafy (mr_ppleafy, from the strip's ballot mr_ppnz), and where one is not, the section four pixels per lane as
// for a tile without a guard bit, with the cover bits' lanes ORed into their reductions' roots.
static std::string prepass_tile(PixelSetup &S, const maray_program &P, const GuardWords &g, const PrepassPlan &pp, bool defer)
{
    Emitter &E = S.E;
    const std::string N = std::to_string(g.n);
    char hex[32];
    snprintf(hex, sizeof hex, "0x%llxull", (1ull << g.n) - 1ull);
    std::string t = std::string(PP_OPEN) +
        "    unsigned mr_ppleafy = 15u;                                             // bit e: pass e runs (a tile off the fast path: all four)\n"
        "    if (mr_fast && mr_wide) {\n"
        "        const unsigned long long mr_ppt = mr_ppnz >> (t * " + g.tw + "u);\n"
        "        mr_ppleafy = ";
    for (uint32_t e = 0; e < 4; e++)
        t += std::string(e ? " | " : "") + "(((mr_ppt >> " + std::to_string(e * g.n) + "u) & " + hex + ") != 0ull ? " + std::to_string(1u << e) + "u : 0u)";
    t += ";\n"
         "    }\n"
         "    if (mr_ppleafy != 15u) {\n";
    if (!pp.roots.empty())
        t += "    // lane l is in rectangle l / 16 of the tile (mr_wide): its rectangle's last word, where the cover bits are\n"
             "    const unsigned mr_ppsrc = ((((t * 4u + (mr_lane >> 4)) * " + N + "u + " + std::to_string(g.n - 1) + "u) & 63u) * 4u);\n";
    bool half[2] = {false, false};
    for (const auto &r : pp.roots) half[(r.second % 64) >= 32] = true;
    if (half[0]) t += "    const unsigned mr_ppw0 = (unsigned)__builtin_amdgcn_ds_bpermute((int)mr_ppsrc, (int)(unsigned)mr_gv);\n";
    if (half[1]) t += "    const unsigned mr_ppw1 = (unsigned)__builtin_amdgcn_ds_bpermute((int)mr_ppsrc, (int)(unsigned)(mr_gv >> 32));\n";
    E.pp_root_or.clear();
    for (size_t k = 0; k < pp.roots.size(); k++) {
        const uint32_t b = pp.roots[k].second % 64;
        snprintf(hex, sizeof hex, "0x%xu", 1u << (b % 32));
        const std::string name = "mr_ppcv" + std::to_string(k);
        t += "    const mr_m " + name + "(mr_ballot((mr_ppw" + (b >= 32 ? "1" : "0") + " & " + hex + ") != 0u));      // the lanes of the rectangles this OR covers\n";
        E.pp_root_or[pp.roots[k].first] = name;
    }
    t += "    const mr_m mr_ppk(mr_ballot(((mr_ppleafy >> (mr_lane >> 4)) & 1u) == 0u));      // the lanes whose pixels are kept\n"
         "    (void)mr_ppk;\n" + wide_open(g);
    std::string &s = E.out;
    s.clear();
    const bool ktab = E.ktab;
    E.ktab = false;             // literals: the constant table stays maray_jit_pixels_rw's, entry for entry
    E.pp_keep = defer ? "mr_ppk" : "";
    E.td = "mr_d"; E.tm = "mr_m"; E.assume_guards_zero = true; E.rplan = nullptr;
    E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
    E.ktab = ktab; E.pp_keep.clear(); E.pp_root_or.clear(); E.assume_guards_zero = false;
    t += s;
    s.clear();
    t += defer_pass(defer) +
         "    const unsigned p0 = mr_cast_u8(o0.a) | (mr_cast_u8(o1.a) << 8) | (mr_cast_u8(o2.a) << 16);\n"
         "    const unsigned p1 = mr_cast_u8(o0.b) | (mr_cast_u8(o1.b) << 8) | (mr_cast_u8(o2.b) << 16);\n"
         "    const unsigned p2 = mr_cast_u8(o0.c) | (mr_cast_u8(o1.c) << 8) | (mr_cast_u8(o2.c) << 16);\n"
         "    const unsigned p3 = mr_cast_u8(o0.d) | (mr_cast_u8(o1.d) << 8) | (mr_cast_u8(o2.d) << 16);\n"
         "    if (mr_ppleafy == 0u) {                                                // no narrow pass: the tile leaves from the registers\n"
         "        mr_u3 d;\n"
         "        d.a = p0 | (p1 << 24); d.b = (p1 >> 8) | (p2 << 16); d.c = (p2 >> 16) | (p3 << 8);\n"
         "        *(mr_u3 *)(rgb8 + (row_px + xa) * 3) = d;\n" +
         tile_end(defer) +
         "        continue;\n"
         "    }\n"
         "    mr_u4 mr_ppq;\n"
         "    mr_ppq.a = p0; mr_ppq.b = p1; mr_ppq.c = p2; mr_ppq.d = p3;\n"
         "    *(mr_u4 *)&mr_tp[mr_wv * 256u + 4u * mr_lane] = mr_ppq;            // what the narrow epilogue reads back; the leafy passes overwrite their 64 entries\n"
         "    __builtin_amdgcn_wave_barrier();                                     // same wavefront: LDS keeps its order\n"
         "    }\n"
         "    }\n" + PP_CLOSE;
    return t;
}

std::string jit_source(const maray_program &P, int min_waves)
{
    validate_program(P);
    const JitKnobs K = jit_knobs();
    PixelSetup S(P, K, min_waves);
    S.E.out += "// generated by libmaray_hip (jit_source.cpp) from a v" + std::to_string(P.version) + " tape: PIXEL section, " +
               std::to_string(P.n_pix_ops) + " ops; general variant " + (jit_wide_general(P, S.n_gwords, K) ? "four pixels per lane" : "one pixel per lane, four passes per tile") + "\n" +
               PIXELS_PROLOGUE;
    pixels_kernel(S, P, K, pixels_head(S.min_waves));
    return S.splice_constants(MR_STORE_RUN);
}

// ---- maray_jit_census --------------------------------------------------------------------------------------------------------
// Folds a rectangle's hit flags into its guard words: out = word & (hits | ~eligible), into the set's second table of words --
// the ROW pass's and the second bounds' words stay what they are (maray_hip_debug_guard_words reads them; the pixel launches
// of a set that has been through its census read `out`).  One work-item per word; the eligible masks are literals of the
// text.  A word without an eligible bit set is copied (and its flags unread).
static std::string census_apply_kernel(const std::vector<uint64_t> &eligible)
{
    std::string s = "extern \"C\" __global__ void __launch_bounds__(256) maray_jit_census_apply(const unsigned long long *__restrict__ gbits, const unsigned char *__restrict__ hits,\n"
                    "                                                                         unsigned long long *__restrict__ out, unsigned n_words)\n{\n"
                    "    const unsigned i = blockIdx.x * 256u + threadIdx.x;                  // (the host keeps the words of a launch below 2^32)\n"
                    "    if (i >= n_words) return;\n"
                    "    unsigned long long mr_el = 0ull;\n"
                    "    switch (i % " + std::to_string(eligible.size()) + "u) {\n";
    for (size_t j = 0; j < eligible.size(); j++) {
        char hex[32];
        snprintf(hex, sizeof hex, "0x%llxull", (unsigned long long)eligible[j]);
        s += "    case " + std::to_string(j) + ": mr_el = " + hex + "; break;\n";
    }
    s += "    }\n"
         "    const unsigned long long word = gbits[i];\n"
         "    if ((word & mr_el) == 0ull) { out[i] = word; return; }\n"
         "    const unsigned long long *h = (const unsigned long long *)(hits + (size_t)i * 64u);      // flag of bit b of word i: byte 64 i + b\n"
         "    unsigned long long m = 0ull;\n"
         "    for (unsigned k = 0; k < 8u; k++) {\n"
         "        const unsigned long long v = h[k];\n"
         "        for (unsigned b = 0; b < 8u; b++) m |= ((v >> (8u * b)) & 1ull) << (8u * k + b);\n"
         "    }\n"
         "    out[i] = word & (m | ~mr_el);\n"
         "}\n";
    return s;
}

// Source of maray_jit_census (and maray_jit_census_apply): the narrow form of maray_jit_pixels with the emitter's census flag
// set (jit_emit.hpp, Emitter::census) -- the prologue, the head, the strip's and the tile's guard words, the pass's tables and
// the section are the very text jit_source() emits, which is the soundness argument: a leaf is evaluated on a rectangle's
// pixels by the instructions that render them.  What differs is what stands here: a tile without a guard bit is left at once
// instead of painted, no pixel is converted or stored, and every leaf a pass enters records, where it is != 0 on a pixel
// inside the picture, a byte flag for its bit in the pass's rectangle (`hits`: 64 x n_gwords bytes per rectangle, indexed
// like the guard words; idempotent plain stores of 1 from lane 0).  The launch is the pixel launch's, over the geometry of a
// kept set.  *eligible: per guard word, the bits a hit decides (see Emitter::census); "" when there are none.
std::string jit_source_census(const maray_program &P, std::vector<uint64_t> *eligible_out, int min_waves)
{
    if (eligible_out) eligible_out->clear();
    validate_program(P);
    const JitKnobs K = jit_knobs();
    PixelSetup S(P, K, min_waves);
    Emitter &E = S.E;
    const GuardWords g(S.n_gwords, S.sub);
    if (!g.n || S.reductions.empty() || jit_wide_general(P, S.n_gwords, K)) return "";
    if (g.per_lane() && g.sub > 1) E.gw_lane_base = "mr_gsub";
    E.census = true;
    E.census_row_params = row_param_mask(P);
    std::string &s = E.out;
    std::string head = pixels_head(S.min_waves);
    head.replace(head.find("maray_jit_pixels("), 17, "maray_jit_census(");
    const char tail[] = "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw)";
    head.replace(head.find(tail), sizeof tail - 1, "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw, unsigned char *__restrict__ mr_hits)");
    s += "// generated by libmaray_hip (jit_source.cpp) from a v" + std::to_string(P.version) + " tape: PIXEL section, " +
         std::to_string(P.n_pix_ops) + " ops; census form: which guarded leaves are != 0 on some pixel of a rectangle\n" +
         PIXELS_PROLOGUE + head + S.texture_loads() + strip_guard_fetch(g) +
         "    (void)rgb8; (void)rgb64;\n"
         "    for (unsigned t = 0; t < tiles; t++) {\n"
         "    const unsigned x0 = (tile0 + t) * 256u;\n"
         "    if (x0 >= w) break;\n"
         "/*MR_KBASE*/" + tile_guard_fetch(g) +
         sky_test(g) + "    continue;\n    }\n"
         "    _Pragma(\"unroll 1\") for (unsigned e = 0; e < 4u; e++) {\n" + PIXELS_PASS_TABLES + pass_guard_words(g) +
         "    const unsigned xw = x0 + 64u * e, x = xw + mr_lane;\n"
         "    const double X = (double)x;\n"
         "    double o0 = 0.0, o1 = 0.0, o2 = 0.0;\n"
         "    float mr_defer = 0.0f;\n"
         "    (void)X; (void)mr_defer;\n"
         "    const mr_mask mr_cin = mr_ballot(x < w);                                 // the lanes inside the picture\n"
         "    // the flags of this pass's rectangle: rectangles are numbered like their guard words\n"
         "    unsigned char *mr_chit = mr_hits + (((size_t)((row_base + r) >> __builtin_ctz(yrows)) * n_tx + tile0 + t) * " + std::to_string(g.sub) + "u + " +
         (g.sub > 1 ? g.esub : std::string("0u")) + ") * " + std::to_string(64 * g.n) + "u;\n";
    {   // the variant of a tile without a guard bit is not part of this kernel, but it comes first in maray_jit_pixels and takes
        // the first entries of the constant table and the first label numbers: emitted and dropped, so that the section below
        // is that kernel's text entry for entry
        const size_t keep = s.size();
        E.td = "mr_d"; E.tm = "mr_m"; E.assume_guards_zero = true; E.rplan = nullptr;
        E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
        s.resize(keep);
    }
    E.td = "double"; E.tm = "mr_mask"; E.assume_guards_zero = false; E.rplan = &S.reductions;
    E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
    s += "    (void)o0; (void)o1; (void)o2;\n"
         "    }\n"
         "    }\n}\n";
    std::vector<uint64_t> eligible(g.n, 0);
    bool any = false;
    for (uint32_t b = 0; b < 64 * g.n && b < E.census_leaf.size(); b++)
        if (E.census_leaf[b] && !(b < E.census_bad.size() && E.census_bad[b])) { eligible[b / 64] |= 1ull << (b % 64); any = true; }
    if (!any) return "";
    s += census_apply_kernel(eligible);
    if (eligible_out) *eligible_out = eligible;
    return S.splice_constants("");
}

// ---- maray_jit_cover, maray_jit_cover_apply, maray_jit_pixels_cov ------------------------------------------------------------------
// Which boolean reductions of a program get a cover bit (Emitter::cover_bit): those the census may decide -- the root in no
// region, at least one guarded leaf on an eligible bit -- as far as the last guard word has bits that no guard uses
// (cover_free_bits, row_reuse.hpp).  A dry run of the census form says which those are and which leaves are tainted.
// bit_of_red: per reduction of the section's RedPlan.
namespace {
struct CoverSetup { CoverPlan plan; std::vector<int32_t> bit_of_red; };

CoverSetup cover_setup(const maray_program &P, const JitKnobs &K)
{
    CoverSetup cs;
    PixelSetup S(P, K, 0);
    Emitter &E = S.E;
    const GuardWords g(S.n_gwords, S.sub);
    if (!g.n || S.reductions.empty() || jit_wide_general(P, S.n_gwords, K)) return cs;
    if (g.per_lane() && g.sub > 1) E.gw_lane_base = "mr_gsub";
    E.census = true;
    E.census_row_params = row_param_mask(P);
    E.td = "double"; E.tm = "mr_mask"; E.assume_guards_zero = false; E.rplan = &S.reductions;
    E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
    auto eligible = [&](uint32_t b) { return b < E.census_leaf.size() && E.census_leaf[b] && !(b < E.census_bad.size() && E.census_bad[b]); };
    std::vector<uint32_t> want;
    for (uint32_t id = 0; id < S.reductions.reds.size(); id++) {
        const RedPlan::Red &red = S.reductions.reds[id];
        bool any = false;
        for (uint32_t b : red.leaf_bit) any |= eligible(b);
        if (red.boolean && any && id < E.red_nested.size() && !E.red_nested[id] && id < E.red_leaf_taint.size()) want.push_back(id);
    }
    // A guard bit belongs to a bound, not to a shape: the lowering interns bounds, so leaves of two reductions (boolean or max)
    // may sit on one bit.  The census ORs the hits of all of them; a cover may clear a bit only for the ONE reduction that is
    // covered, so a bit with leaves in more than one reduction is never cleared (the covered OR still skips its own loops)
    std::vector<uint32_t> owners(64 * g.n, 0);
    for (const RedPlan::Red &red : S.reductions.reds)
        for (uint32_t b : red.leaf_bit) if (b < owners.size()) owners[b]++;
    std::vector<int32_t> bits(want.size(), -1);
    const uint32_t got = cover_free_bits(S.plan.n_pos, g.n, (uint32_t)want.size(), bits.data());
    cs.bit_of_red.assign(S.reductions.reds.size(), -1);
    cs.plan.n_words = g.n;
    for (uint32_t k = 0; k < got; k++) {
        const RedPlan::Red &red = S.reductions.reds[want[k]];
        CoverPlan::Red r;
        r.bit = bits[k]; r.root = red.root; r.leaf_end = red.leaf_end; r.leaf_bit = red.leaf_bit;
        r.leaf_taint = E.red_leaf_taint[want[k]];
        r.leaf_taint.resize(red.leaf_bit.size(), 1);
        for (uint32_t b : red.leaf_bit) r.leaf_eligible.push_back(eligible(b) && b < owners.size() && owners[b] == 1);
        cs.plan.reds.push_back(r);
        cs.bit_of_red[want[k]] = bits[k];
    }
    return cs;
}
}   // namespace

CoverPlan jit_cover_plan(const maray_program &P)
{
    validate_program(P);
    return cover_setup(P, jit_knobs()).plan;
}

// Writes a set's third table of words: the census'd words, and for each (rectangle, reduction) whose flags say "seen and
// no pixel missed" the reduction's cover bit set and its leaf bits that are census-eligible and carry no leaf of another reduction -- those gate nothing else -- cleared.  One
// work-item per word; the masks are literals of the text.  *n_set counts the cover bits set (the host launches
// maray_jit_pixels_cov over the table only if there are any).
static std::string cover_apply_kernel(const CoverPlan &cp)
{
    const uint32_t nw = cp.n_words, nc = (uint32_t)cp.reds.size();
    std::string s = "extern \"C\" __global__ void __launch_bounds__(256) maray_jit_cover_apply(const unsigned long long *__restrict__ cbits, const unsigned char *__restrict__ flags,\n"
                    "                                                                        unsigned long long *__restrict__ out, unsigned n_words, unsigned *__restrict__ n_set)\n{\n"
                    "    const unsigned i = blockIdx.x * 256u + threadIdx.x;                  // (the host keeps the words of a launch below 2^32)\n"
                    "    if (i >= n_words) return;\n"
                    "    const unsigned char *f = flags + (size_t)(i / " + std::to_string(nw) + "u) * " + std::to_string(2 * nc) + "u;      // the flags of the word's rectangle\n"
                    "    unsigned long long word = cbits[i];\n"
                    "    switch (i % " + std::to_string(nw) + "u) {\n";
    for (uint32_t w = 0; w < nw; w++) {
        std::string body;
        for (uint32_t j = 0; j < nc; j++) {
            uint64_t clear = 0, set = 0;
            for (size_t k = 0; k < cp.reds[j].leaf_bit.size(); k++)
                if (cp.reds[j].leaf_eligible[k] && cp.reds[j].leaf_bit[k] / 64 == w) clear |= 1ull << (cp.reds[j].leaf_bit[k] % 64);
            if ((uint32_t)cp.reds[j].bit / 64 == w) set = 1ull << ((uint32_t)cp.reds[j].bit % 64);
            if (!clear && !set) continue;
            char hex[96];
            snprintf(hex, sizeof hex, "word = (word & ~0x%llxull) | 0x%llxull;", (unsigned long long)clear, (unsigned long long)set);
            body += "        if (f[" + std::to_string(2 * j) + "] && !f[" + std::to_string(2 * j + 1) + "]) { " + hex + (set ? " atomicAdd(n_set, 1u);" : "") + " }\n";
        }
        if (!body.empty()) s += "    case " + std::to_string(w) + ":\n" + body + "        break;\n";
    }
    s += "    }\n"
         "    out[i] = word;\n"
         "}\n";
    return s;
}

// Source of the cover module: maray_jit_pixels_cov, maray_jit_cover and maray_jit_cover_apply; "" when the program gets no
// cover bit.  All three from the generator of maray_jit_pixels -- the prologue, the head, the guard words' fetches, the pass's
// tables and the section are that kernel's text, and the constant table (one for the module) is that kernel's entry for entry:
//  * maray_jit_pixels_cov is maray_jit_pixels with one scalar test at the root of a reduction that has a cover bit: the bit
//    set in the pass's guard word, the OR is MR_ALL and its loops are not entered;
//  * maray_jit_cover is the narrow form without stores, like maray_jit_census, over the set's census'd words: it records per
//    (rectangle, reduction) `seen` and `miss` (Emitter::cover), 2 bytes per reduction with a bit, rectangles numbered like
//    their guard words.
// Exactness: OR on lane masks is associative and commutative; with the bit set the untainted leaves alone are 1 on every
// pixel of the rectangle inside the picture under the set's key, so the OR is all-ones there whatever the leaves that are
// not entered would have computed; lanes outside the picture are never stored.
std::string jit_source_cover(const maray_program &P, CoverPlan *plan_out, int min_waves)
{
    if (plan_out) *plan_out = CoverPlan();
    validate_program(P);
    const JitKnobs K = jit_knobs();
    const CoverSetup cs = cover_setup(P, K);
    if (cs.plan.reds.empty()) return "";
    PixelSetup S(P, K, min_waves);
    Emitter &E = S.E;
    const GuardWords g(S.n_gwords, S.sub);
    E.cover_bit = cs.bit_of_red;
    E.census_row_params = row_param_mask(P);
    std::string &s = E.out;
    s += "// generated by libmaray_hip (jit_source.cpp) from a v" + std::to_string(P.version) + " tape: PIXEL section, " +
         std::to_string(P.n_pix_ops) + " ops; cover forms: " + std::to_string(cs.plan.reds.size()) + " OR(s) of shapes may be known to be 1 on every pixel of a rectangle\n" +
         PIXELS_PROLOGUE;
    const size_t ktab0 = E.ktab_vals.size();
    std::string head = pixels_head(S.min_waves);
    head.replace(head.find("maray_jit_pixels("), 17, "maray_jit_pixels_cov(");
    E.use_cover = true;
    pixels_kernel(S, P, K, head);
    E.use_cover = false;
    // maray_jit_cover: the constant table and the label numbers start over, so that its section is that kernel's text too
    const std::vector<double> table = E.ktab_vals;
    E.ktab_vals.resize(ktab0);
    E.ktab_block.clear();
    E.red_serial = 0;
    head = pixels_head(S.min_waves);
    head.replace(head.find("maray_jit_pixels("), 17, "maray_jit_cover(");
    const char tail[] = "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw)";
    head.replace(head.find(tail), sizeof tail - 1, "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw, unsigned char *__restrict__ mr_cover)");
    s += "\n" + head + S.texture_loads() + strip_guard_fetch(g) +
         "    (void)rgb8; (void)rgb64;\n"
         "    for (unsigned t = 0; t < tiles; t++) {\n"
         "    const unsigned x0 = (tile0 + t) * 256u;\n"
         "    if (x0 >= w) break;\n"
         "/*MR_KBASE*/" + tile_guard_fetch(g) +
         sky_test(g) + "    continue;\n    }\n"
         "    _Pragma(\"unroll 1\") for (unsigned e = 0; e < 4u; e++) {\n" + PIXELS_PASS_TABLES + pass_guard_words(g) +
         "    const unsigned xw = x0 + 64u * e, x = xw + mr_lane;\n"
         "    const double X = (double)x;\n"
         "    double o0 = 0.0, o1 = 0.0, o2 = 0.0;\n"
         "    float mr_defer = 0.0f;\n"
         "    (void)X; (void)mr_defer;\n"
         "    const mr_mask mr_cin = mr_ballot(x < w);                                 // the lanes inside the picture\n"
         "    // the flags of this pass's rectangle: rectangles are numbered like their guard words\n"
         "    unsigned char *mr_cvf = mr_cover + (((size_t)((row_base + r) >> __builtin_ctz(yrows)) * n_tx + tile0 + t) * " + std::to_string(g.sub) + "u + " +
         (g.sub > 1 ? g.esub : std::string("0u")) + ") * " + std::to_string(2 * cs.plan.reds.size()) + "u;\n";
    {   // (the variant of a tile without a guard bit: emitted and dropped, as in jit_source_census)
        const size_t keep = s.size();
        E.td = "mr_d"; E.tm = "mr_m"; E.assume_guards_zero = true; E.rplan = nullptr;
        E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
        s.resize(keep);
    }
    E.cover = true;
    E.td = "double"; E.tm = "mr_mask"; E.assume_guards_zero = false; E.rplan = &S.reductions;
    E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
    E.cover = false;
    s += "    (void)o0; (void)o1; (void)o2;\n"
         "    }\n"
         "    }\n}\n";
    if (E.ktab_vals.size() != table.size() || memcmp(E.ktab_vals.data(), table.data(), table.size() * sizeof(double)) != 0)
        throw Error{MARAY_E_INTERNAL, "the cover kernels disagree about the constant table"};
    s += cover_apply_kernel(cs.plan);
    if (plan_out) *plan_out = cs.plan;
    return S.splice_constants(MR_STORE_RUN);
}

// ---- maray_jit_rowscan, maray_jit_pixels_rw ------------------------------------------------------------------------------------
// The row words of a program: a rectangle's guard words refined row by row.  The cover's words say what holds
// on EVERY row of a rectangle; a shape whose edge is horizontal in the middle of a band leaves its rectangles mixed although
// each single row is all inside or all outside.  maray_jit_rowscan forms, per (rectangle, row), the band's words without the
// eligible leaf bits whose leaf is 0 on the row and with the cover bits of the ORs whose untainted leaves cover the row -- the
// census's rule and the cover's, unchanged, one row at a time; maray_jit_pixels_rw reads them for the rectangles whose last
// word carries the ROW FLAG, one more free bit of that word (cover_free_bits), set by maray_jit_rowscan_apply (rowwords.hip)
// where enough rows differ from the band.
//
// Only for programs whose rectangles are one pass wide (64 pixels: a pass of the scan sees all of its (rectangle, row) and
// needs no flags in memory) and whose words are fetched per strip (<= GW_INLINE_MAX): the others stay on the kernels above.
// "" when the program gets no row words: no reduction, no eligible bit, no spare bit for the flag.
namespace {
// the strip's guard fetch of maray_jit_pixels_rw: strip_guard_fetch()'s, then each lane learns from its rectangle's last word
// whether the rectangle is flagged (one cross-lane read), and where some lane's is (a ballot: wave-uniform) those lanes take
// their word of this row from mr_rwords.  Row words are stored without the flag: it reaches no bit test.  A strip without a
// flagged rectangle executes no load.
std::string strip_guard_fetch_rw(const GuardWords &g, uint32_t flag_bit)
{
    const uint32_t fb = flag_bit % 64;
    char hex[24];
    snprintf(hex, sizeof hex, "0x%xu", 1u << (fb % 32));
    return "    const unsigned long long mr_gbase0 = (unsigned long long)(gbits + ((size_t)((row_base + r) >> __builtin_ctz(yrows)) * n_tx + tile0) * " + g.tw + "u);\n"
           "    const unsigned mr_gn = (n_tx - tile0 < tiles ? n_tx - tile0 : tiles) * " + g.tw + "u;       // <= 64: the host bounds `tiles`\n"
           "    unsigned long long mr_gv = mr_lane < mr_gn ? ((const unsigned long long *)mr_gbase0)[mr_lane] : 0ull;\n"
           "    {   // row words: lane i holds word i % " + g.nw + " of rectangle i / " + g.nw + " of the strip; the flag sits in that rectangle's last word\n"
           "        const unsigned mr_rwr = mr_lane / " + g.nw + "u, mr_rwl = mr_rwr * " + g.nw + "u + " + std::to_string(g.n - 1) + "u;\n"
           "        const unsigned mr_rwf = (unsigned)__builtin_amdgcn_ds_bpermute((int)((mr_rwl & 63u) * 4u), (int)(unsigned)(mr_gv" + (fb >= 32 ? " >> 32" : "") + "));\n"
           "        const bool mr_rwt = mr_lane < mr_gn && (mr_rwf & " + hex + ") != 0u;\n"
           "        if (mr_ballot(mr_rwt) != 0ull) {                                      // wave-uniform: some rectangle of the strip has row words\n"
           "            if (mr_rwt) mr_gv = mr_rwords[(((size_t)(row_base + r) * n_tx + tile0) * " + std::to_string(g.sub) + "u + mr_rwr) * " + g.nw + "u + (mr_lane - mr_rwr * " + g.nw + "u)];\n"
           "        }\n"
           "    }\n" +
           (g.sub > 1 ? "    const unsigned long long mr_gnz = mr_ballot(mr_gv != 0ull);            // which of the strip's words have a bit set\n" : "");
}

struct RowWordsSetup { CoverSetup cs; std::vector<uint64_t> eligible; int32_t flag_bit = -1; };

RowWordsSetup rowwords_setup(const maray_program &P, const JitKnobs &K)
{
    RowWordsSetup rs;
    const uint32_t n_gwords = jit_guard_words(P, K);
    const GuardGeom geom = jit_guard_geom(P, K);
    if (!n_gwords || n_gwords > GW_INLINE_MAX || geom.gw != 64u || geom.gh < 2u) return rs;
    if (jit_source_census(P, &rs.eligible).empty() || rs.eligible.size() != n_gwords) { rs.eligible.clear(); return rs; }
    rs.cs = cover_setup(P, K);
    // the flag: the free bit behind the cover bits, if the last word has one more
    const uint32_t n_cover = (uint32_t)rs.cs.plan.reds.size();
    std::vector<int32_t> bits(n_cover + 1, -1);
    const uint32_t n_pos = jit_guard_plan(P).n_pos;
    if (cover_free_bits(n_pos, n_gwords, n_cover + 1, bits.data()) == n_cover + 1) rs.flag_bit = bits[n_cover];
    for (uint32_t k = 0; k < n_cover; k++) if (rs.cs.plan.reds[k].bit != bits[k]) rs.flag_bit = -1;     // (the cover's bits are the first granted)
    return rs;
}
}   // namespace

RowWordsPlan jit_rowwords_plan(const maray_program &P)
{
    validate_program(P);
    const RowWordsSetup rs = rowwords_setup(P, jit_knobs());
    RowWordsPlan rp;
    if (rs.flag_bit < 0) return rp;
    rp.flag_bit = rs.flag_bit; rp.n_words = (uint32_t)rs.eligible.size(); rp.n_cover = (uint32_t)rs.cs.plan.reds.size();
    return rp;
}

std::string jit_source_rowwords(const maray_program &P, RowWordsPlan *plan_out, int min_waves)
{
    if (plan_out) *plan_out = RowWordsPlan();
    validate_program(P);
    const JitKnobs K = jit_knobs();
    const RowWordsSetup rs = rowwords_setup(P, K);
    if (rs.flag_bit < 0) return "";
    const CoverSetup &cs = rs.cs;
    PixelSetup S(P, K, min_waves);
    Emitter &E = S.E;
    const GuardWords g(S.n_gwords, S.sub);
    if (!g.in_sgprs || g.sub != 4 || S.reductions.empty() || jit_wide_general(P, S.n_gwords, K)) return "";
    E.cover_bit = cs.bit_of_red;
    E.census_row_params = row_param_mask(P);
    std::string &s = E.out;
    s += "// generated by libmaray_hip (jit_source.cpp) from a v" + std::to_string(P.version) + " tape: PIXEL section, " +
         std::to_string(P.n_pix_ops) + " ops; row words: the guard words of a rectangle, refined row by row; the row flag is bit " + std::to_string(rs.flag_bit) + "\n" +
         PIXELS_PROLOGUE;
    const size_t ktab0 = E.ktab_vals.size();
    const char tail[] = "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw)";
    std::string head = pixels_head(S.min_waves);
    head.replace(head.find("maray_jit_pixels("), 17, "maray_jit_pixels_rw(");
    head.replace(head.find(tail), sizeof tail - 1, "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw, const unsigned long long *__restrict__ mr_rwords)");
    const std::string fetch = strip_guard_fetch_rw(g, (uint32_t)rs.flag_bit);
    E.use_cover = true;
    pixels_kernel(S, P, K, head, &fetch);
    E.use_cover = false;
    // maray_jit_rowscan: the constant table and the label numbers start over, so that its section is that kernel's text too
    const std::vector<double> table = E.ktab_vals;
    E.ktab_vals.resize(ktab0);
    E.ktab_block.clear();
    E.red_serial = 0;
    head = pixels_head(S.min_waves);
    head.replace(head.find("maray_jit_pixels("), 17, "maray_jit_rowscan(");
    head.replace(head.find(tail), sizeof tail - 1, "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw, unsigned long long *__restrict__ mr_rwords, unsigned char *__restrict__ mr_changed)");
    // the leaf bits of the reductions, per word: a rectangle without one has nothing to refine
    std::vector<uint64_t> redmask(g.n, 0);
    for (const RedPlan::Red &red : S.reductions.reds) for (uint32_t b : red.leaf_bit) if (b / 64 < g.n) redmask[b / 64] |= 1ull << (b % 64);
    auto hex64 = [](uint64_t v) { char h[32]; snprintf(h, sizeof h, "0x%llxull", (unsigned long long)v); return std::string(h); };
    std::string lane_mask = "    unsigned long long mr_rwm = 0ull;\n    switch (mr_lane % " + g.nw + "u) {\n", any_red, decl;
    for (uint32_t j = 0; j < g.n; j++) {
        const std::string k = std::to_string(j);
        lane_mask += "    case " + k + ": mr_rwm = " + hex64(redmask[j]) + "; break;\n";
        any_red += std::string(j ? " | " : "") + "(gq" + k + " & " + hex64(redmask[j]) + ")";
        decl += "    mr_mask mr_rwh" + k + " = 0ull;\n";
    }
    s += "\n" + head + S.texture_loads() + strip_guard_fetch(g) +
         "    (void)rgb8; (void)rgb64;\n" + lane_mask + "    }\n"
         "    if (mr_ballot((mr_gv & mr_rwm) != 0ull) == 0ull) return;                  // no rectangle of the strip holds a leaf bit of a reduction\n"
         "    for (unsigned t = 0; t < tiles; t++) {\n"
         "    const unsigned x0 = (tile0 + t) * 256u;\n"
         "    if (x0 >= w) break;\n"
         "/*MR_KBASE*/" + tile_guard_fetch(g) +
         sky_test(g) + "    continue;\n    }\n"
         "    _Pragma(\"unroll 1\") for (unsigned e = 0; e < 4u; e++) {\n" + PIXELS_PASS_TABLES + pass_guard_words(g) +
         "    const unsigned xw = x0 + 64u * e, x = xw + mr_lane;\n"
         "    const double X = (double)x;\n"
         "    double o0 = 0.0, o1 = 0.0, o2 = 0.0;\n"
         "    float mr_defer = 0.0f;\n"
         "    (void)X; (void)mr_defer;\n"
         "    const mr_mask mr_cin = mr_ballot(x < w);                                 // the lanes inside the picture\n"
         "    if (mr_cin == 0ull) continue;                                            // no pixel of the rectangle on this row: the band's words stand\n"
         "    if ((" + any_red + ") == 0ull) continue;                                 // nothing to refine\n" +
         decl +
         "    unsigned mr_rwcv = 0u;\n";
    {   // (the variant of a tile without a guard bit: emitted and dropped, as in jit_source_census)
        const size_t keep = s.size();
        E.td = "mr_d"; E.tm = "mr_m"; E.assume_guards_zero = true; E.rplan = nullptr;
        E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
        s.resize(keep);
    }
    E.census = true; E.cover = true; E.rowscan = true;
    E.td = "double"; E.tm = "mr_mask"; E.assume_guards_zero = false; E.rplan = &S.reductions;
    E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
    E.census = false; E.cover = false; E.rowscan = false;
    s += "    (void)o0; (void)o1; (void)o2;\n"
         "    // the row's words: the band's, without the eligible bits of leaves that are 0 on the row ...\n";
    std::string differ, stores;
    for (uint32_t j = 0; j < g.n; j++) {
        const std::string k = std::to_string(j);
        s += "    mr_mask mr_rw" + k + " = gq" + k + " & (mr_rwh" + k + " | " + hex64(~rs.eligible[j]) + ");\n";
        differ += std::string(j ? " || " : "") + "mr_rw" + k + " != gq" + k;
        stores += "        mr_rwq[" + k + "] = mr_rw" + k + ";\n";
    }
    s += "    // ... and, where the untainted leaves of an OR cover the row, with its cover bit in place of its own eligible leaf bits\n";
    for (uint32_t j = 0; j < cs.plan.reds.size(); j++) {
        const CoverPlan::Red &red = cs.plan.reds[j];
        std::vector<uint64_t> clear(g.n, 0);
        for (size_t k = 0; k < red.leaf_bit.size(); k++) if (red.leaf_eligible[k]) clear[red.leaf_bit[k] / 64] |= 1ull << (red.leaf_bit[k] % 64);
        s += "    if ((mr_rwcv & " + std::to_string(1u << j) + "u) != 0u) {\n";
        for (uint32_t wd = 0; wd < g.n; wd++) {
            const uint64_t set = (uint32_t)red.bit / 64 == wd ? 1ull << ((uint32_t)red.bit % 64) : 0ull;
            if (clear[wd] || set) s += "        mr_rw" + std::to_string(wd) + " = (mr_rw" + std::to_string(wd) + " & " + hex64(~clear[wd]) + ") | " + hex64(set) + ";\n";
        }
        s += "    }\n";
    }
    s += "    if (mr_lane == 0u) {                                                     // idempotent plain stores, one lane\n"
         "        const size_t mr_rwi = ((size_t)(row_base + r) * n_tx + tile0 + t) * 4u + e;      // (row of the call, rectangle)\n"
         "        unsigned long long *mr_rwq = mr_rwords + mr_rwi * " + g.nw + "u;\n" + stores +
         "        mr_changed[((((size_t)((row_base + r) >> __builtin_ctz(yrows)) * n_tx + tile0 + t) * 4u + e) * yrows) + ((row_base + r) & (yrows - 1u))] = (" + differ + ") ? 1 : 0;\n"
         "    }\n"
         "    }\n"
         "    }\n}\n";
    if (E.ktab_vals.size() != table.size() || memcmp(E.ktab_vals.data(), table.data(), table.size() * sizeof(double)) != 0)
        throw Error{MARAY_E_INTERNAL, "the row-word kernels disagree about the constant table"};
    if (plan_out) { plan_out->flag_bit = rs.flag_bit; plan_out->n_words = g.n; plan_out->n_cover = (uint32_t)cs.plan.reds.size(); }
    return S.splice_constants(MR_STORE_RUN);
}

// ---- maray_jit_pixels_pp -----------------------------------------------------------------------------------------------------------
// Source of the pre-pass module: maray_jit_pixels_pp, whose text is maray_jit_pixels_rw's plus the lines
// between PP_OPEN and PP_CLOSE, every one of which ends up carrying "mr_pp".  A rectangle whose guard words are zero apart
// from cover bits is LEAFLESS: a narrow pass over it enters no leaf, computes every row-guarded region as +0.0, every
// uncovered reduction as its free leaves and every covered OR as MR_ALL -- and costs its table copies, its six v_readlane,
// the skeleton of its reductions, its conversions and its LDS write all the same.  On the fast RGB8 path a busy tile with a
// leafless rectangle renders those rectangles in ONE wide pre-pass, the section as for a tile without a guard bit with the
// covered rectangles' lanes ORed in at the roots, leaves the packed pixels where the narrow passes leave theirs, and the
// narrow loop runs the leafy passes only.  Exact for the sky variant's reasons: OR on masks is associative and commutative,
// a clear bit means +0.0 on the whole rectangle, an evaluator may ignore any SKIP op.
// For the programs that get row words (rowwords_setup) whose cover bits and row flag sit in the last guard word; "" otherwise.
std::string jit_source_prepass(const maray_program &P, int min_waves)
{
    validate_program(P);
    const JitKnobs K = jit_knobs();
    const RowWordsSetup rs = rowwords_setup(P, K);
    if (rs.flag_bit < 0) return "";
    const CoverSetup &cs = rs.cs;
    PixelSetup S(P, K, min_waves);
    Emitter &E = S.E;
    const GuardWords g(S.n_gwords, S.sub);
    if (!g.in_sgprs || g.sub != 4 || S.reductions.empty() || jit_wide_general(P, S.n_gwords, K)) return "";
    if ((uint32_t)rs.flag_bit / 64 != g.n - 1) return "";
    // per word: the bits that make a rectangle leafy -- all but the cover bits and, in words that come from the band's table,
    // the row flag (row words are stored without it)
    PrepassPlan pp;
    std::vector<uint64_t> leafy(g.n, ~0ull);
    leafy[g.n - 1] &= ~(1ull << ((uint32_t)rs.flag_bit % 64));
    for (uint32_t id = 0; id < S.reductions.reds.size() && id < cs.bit_of_red.size(); id++) {
        const int32_t bit = cs.bit_of_red[id];
        if (bit < 0) continue;
        if ((uint32_t)bit / 64 != g.n - 1 || !S.reductions.reds[id].boolean) return "";
        pp.roots.emplace_back(S.reductions.reds[id].root, (uint32_t)bit);
        leafy[g.n - 1] &= ~(1ull << ((uint32_t)bit % 64));
    }
    E.cover_bit = cs.bit_of_red;
    E.census_row_params = row_param_mask(P);
    std::string &s = E.out;
    s += "// generated by libmaray_hip (jit_source.cpp) from a v" + std::to_string(P.version) + " tape: PIXEL section, " +
         std::to_string(P.n_pix_ops) + " ops; row words: the guard words of a rectangle, refined row by row; the row flag is bit " + std::to_string(rs.flag_bit) + "\n"
         "// mr_pp: with a wide pre-pass of a busy tile's leafless rectangles\n" +
         PIXELS_PROLOGUE;
    const char tail[] = "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw)";
    std::string head = pixels_head(S.min_waves);
    head.replace(head.find("maray_jit_pixels("), 17, "maray_jit_pixels_pp(");
    head.replace(head.find(tail), sizeof tail - 1, "const unsigned *__restrict__ row_order, unsigned rows, unsigned rpw, const unsigned long long *__restrict__ mr_rwords)");
    std::string fetch = strip_guard_fetch_rw(g, (uint32_t)rs.flag_bit) + PP_OPEN +
                        "    unsigned long long mr_ppm = 0ull;                                      // per lane (word lane % " + g.nw + " of its rectangle): the bits that make a rectangle leafy\n"
                        "    switch (mr_lane % " + g.nw + "u) {\n";
    for (uint32_t j = 0; j < g.n; j++) {
        char hex[32];
        snprintf(hex, sizeof hex, "0x%llxull", (unsigned long long)leafy[j]);
        fetch += "    case " + std::to_string(j) + ": mr_ppm = " + hex + "; break;\n";
    }
    fetch += "    }\n"
             "    const unsigned long long mr_ppnz = mr_ballot((mr_gv & mr_ppm) != 0ull);      // which of the strip's words hold such a bit\n" + std::string(PP_CLOSE);
    E.use_cover = true;
    pixels_kernel(S, P, K, head, &fetch, &pp);
    E.use_cover = false;
    const std::string text = S.splice_constants(MR_STORE_RUN);
    // every line between the sentinels carries the marker
    std::string out;
    bool inside = false;
    for (size_t at = 0; at < text.size();) {
        const size_t nl = text.find('\n', at), end = nl == std::string::npos ? text.size() : nl;
        std::string line = text.substr(at, end - at);
        if (line.find("/*mr_pp{*/") != std::string::npos) inside = true;
        if (inside && line.find("mr_pp") == std::string::npos) line += "      // mr_pp";
        if (line.find("/*mr_pp}*/") != std::string::npos) inside = false;
        out += line + "\n";
        at = end + 1;
    }
    return out;
}

// ---- maray_jit_pixels_ss ---------------------------------------------------------------------------------------------------------
static const char SAMPLES_PROLOGUE[] =
    "#define MR_VEC4 1\n"
    "#include \"device_math.h\"\n"
    "typedef const __attribute__((address_space(4))) double *mr_kptr;\n"
    "typedef const __attribute__((address_space(4))) unsigned long long *mr_gptr;\n"
    "__device__ inline mr_mask mr_lane64(unsigned long long v, unsigned lane)\n"
    "{\n"
    "    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, (int)lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), (int)lane);\n"
    "    return ((mr_mask)hi << 32) | lo;\n"
    "}\n/*MR_KTAB*/\n";

// w, y0, blk_rows, blk_stride: samples; row_base + blockIdx.y: the OUTPUT row of the call; yvals, gbits and rgb8 belong to the whole call
static std::string samples_head(int min_waves)
{
    return "extern \"C\" __global__ void __launch_bounds__(256, " + std::to_string(min_waves) +
         ") maray_jit_pixels_ss(unsigned char *__restrict__ rgb8, const double *__restrict__ yvals, const MarayTex *__restrict__ tex,\n"
         "                                                                       const unsigned long long *__restrict__ gbits, unsigned n_tx,\n"
         "                                                                       unsigned w, unsigned y0, unsigned n_yvals, unsigned tiles,\n"
         "                                                                       unsigned blk_rows, unsigned blk_stride, unsigned row_base, unsigned yrows,\n"
         "                                                                       unsigned w_out)\n{\n"
         "    const unsigned mr_wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), mr_lane = threadIdx.x & 63u;\n"
         "    const unsigned tile0 = (blockIdx.x * 4u + mr_wv) * tiles;\n"
         "    if (tile0 >= n_tx) return;\n"
         "    const unsigned r = row_base + blockIdx.y;                               // output row of the call\n"
         "    (void)tex; (void)gbits; (void)yrows;\n";
}

// Source of the supersampling PIXEL kernel, maray_jit_pixels_ss (include/maray_hip.h, supersampling): the
// narrow form of jit_source -- one sample per lane, the section's guard tests and branch tables as they are -- over the k w x k h
// sample grid of a supersampled scene.  A wavefront owns a strip of `tiles` tiles of 256 sample columns of one OUTPUT row
// (blockIdx.y); per pass of 64 sample columns it walks the k sample rows of that output row, each with its own y values
// and the guard words of its own group of rows (a group may end inside a pixel's k rows), and adds the cast samples of a
// lane in integer registers.  k divides 64: a pixel's k columns are k neighbouring lanes, summed across by shuffles; the
// group's first lane stores the pixel's mean.  k is a literal of the source, so it is part of the code object's key.
// Nothing is deferred to the interpreter: an unbounded Sin takes its full reduction here.  What differs from jit_source is
// what stands here: one kernel form, every guard word of the rectangle at hand a named SGPR pair loaded per sample row and
// pass (scalar loads), the sums and the store.
std::string jit_source_samples(const maray_program &P, uint32_t k, int min_waves)
{
    validate_program(P);
    if (k != 2 && k != 4 && k != 8) throw Error{MARAY_E_ARG, "supersampling kernels exist for k = 2, 4 and 8"};
    // This kernel was written without the ablation knobs of the section's text, and its pinned sources
    // (tests/golden/jit_source_hashes.json) say it still ignores them: the defaults, whatever the environment says.  The
    // knobs of the guards (MARAY_JIT_ROW_GUARDS, MARAY_JIT_GUARD_W / _H) are the ROW kernel's too and are honoured.
    JitKnobs K = jit_knobs();
    K.min_region = JitKnobs().min_region; K.fuse_cmp = true; K.reduce = true; K.texel_once = true;
    PixelSetup S(P, K, min_waves);
    Emitter &E = S.E;
    E.no_defer = true;
    if (S.n_gwords) E.gw_inline_max = S.n_gwords;
    const std::string Ks = std::to_string(k), nw = std::to_string(S.n_gwords), half = std::to_string(k * k / 2), shift = std::to_string(2 * (k == 2 ? 1 : k == 4 ? 2 : 3));
    const std::string esub = S.sub == 1 ? "0u" : S.sub == 2 ? "(e >> 1u)" : "e";       // rectangle of pass e inside its tile
    std::string &s = E.out;
    s += "// generated by libmaray_hip (jit_source.cpp) from a v" + std::to_string(P.version) + " tape: PIXEL section, " +
         std::to_string(P.n_pix_ops) + " ops; supersampling " + Ks + " x " + Ks + " samples per pixel, one sample per lane\n" +
         SAMPLES_PROLOGUE + samples_head(S.min_waves) + S.texture_loads() +
         "    for (unsigned t = 0; t < tiles; t++) {\n"
         "    const unsigned x0 = (tile0 + t) * 256u;\n"
         "    if (x0 >= w) break;\n"
         "/*MR_KBASE*/"
         "    _Pragma(\"unroll 1\") for (unsigned e = 0; e < 4u; e++) {\n"
         "    const unsigned x = x0 + 64u * e + mr_lane;                             // sample column\n"
         "    const double X = (double)x;\n"
         "    unsigned mr_s01 = 0u, mr_s2 = 0u;                                       // R | G << 16, B: at most 255 k^2 <= 16320 each\n"
         "    (void)X;\n"
         "    _Pragma(\"unroll 1\") for (unsigned mr_j = 0; mr_j < " + Ks + "u; mr_j++) {\n"
         "    const unsigned rs = r * " + Ks + "u + mr_j;                                 // sample row of the call\n"
         "    const double Y = (double)(blk_stride == 0u ? y0 + rs : y0 + (rs / blk_rows) * blk_stride + rs % blk_rows);\n"
         "    (void)Y;\n"
         "    unsigned long long mr_ybase = (unsigned long long)(yvals + (size_t)rs * n_yvals);\n" + PASS_TABLES;
    if (S.n_gwords) {
        s += "    unsigned long long mr_gb = (unsigned long long)(gbits + (((size_t)(rs >> __builtin_ctz(yrows)) * n_tx + tile0 + t) * " + std::to_string(S.sub) +
             "u + " + esub + ") * " + nw + "u);\n"
             "    asm volatile(\"\" : \"+s\"(mr_gb));\n"
             "    const mr_gptr mr_g = (mr_gptr)mr_gb;\n";
        for (uint32_t j = 0; j < S.n_gwords; j++) s += "    mr_mask gq" + std::to_string(j) + " = mr_g[" + std::to_string(j) + "];\n";
    }
    s += "    double o0 = 0.0, o1 = 0.0, o2 = 0.0;\n"
         "    float mr_defer = 0.0f;\n"
         "    (void)mr_defer;\n";
    E.td = "double"; E.tm = "mr_mask"; E.rplan = &S.reductions;
    E.section(P.pix_ops, P.n_pix_ops, P.n_pix_slots, true, "v");
    s += "    mr_s01 += mr_cast_u8(o0) | (mr_cast_u8(o1) << 16);\n"
         "    mr_s2 += mr_cast_u8(o2);\n"
         "    }\n"
         "    // a pixel's k sample columns are k neighbouring lanes: their sums, across lanes without memory\n"
         "    _Pragma(\"unroll\") for (unsigned m = 1u; m < " + Ks + "u; m <<= 1) {\n"
         "        mr_s01 += (unsigned)__shfl_xor((int)mr_s01, (int)m);\n"
         "        mr_s2 += (unsigned)__shfl_xor((int)mr_s2, (int)m);\n"
         "    }\n"
         "    const unsigned xo = x / " + Ks + "u;\n"
         "    if ((mr_lane & " + std::to_string(k - 1) + "u) == 0u && xo < w_out) {\n"
         "        unsigned char *q = rgb8 + ((size_t)r * w_out + xo) * 3;\n"
         "        q[0] = (unsigned char)(((mr_s01 & 0xFFFFu) + " + half + "u) >> " + shift + "u);\n"
         "        q[1] = (unsigned char)(((mr_s01 >> 16) + " + half + "u) >> " + shift + "u);\n"
         "        q[2] = (unsigned char)((mr_s2 + " + half + "u) >> " + shift + "u);\n"
         "    }\n"
         "    }\n"
         "    }\n}\n";
    return S.splice_constants("");
}

}   // namespace maray
