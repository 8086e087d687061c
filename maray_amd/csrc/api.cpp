// api.cpp — extern "C" boundary of libmaray_hip.so (product code).
// Every function converts maray::Error into a code + thread-local message and
// never lets an exception cross the ABI.
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "apng_device.hpp"
#include "y4m_device.hpp"
#include "backend.hpp"
#include "expr.hpp"
#include "filter.hpp"
#include "lower.hpp"
#include "maray_hip.h"
#include "maray_transfer_table.h"
#include "png_device.hpp"
#include "shutter.hpp"

using namespace maray;

struct maray_scene {
    Scene s;
    // 128-bit name of the scene's program: what maray_gen_to_image remembers a scene's tape and contexts under.  A scene read from
    // bytes is named by the hash of those bytes (without the header: the size is not part of a program); a rescale of a named
    // scene folds its factors into the name (load, rescale, render is what the CLI and an embedding do: re-encoding 88,000
    // nodes to name them cost the first call of chess 3-4 ms); every other call that changes the scene drops the name, and
    // the next use hashes the scene's encoding (what `save` would write).  Two names for one program are a miss in the
    // cache, nothing worse.
    std::mutex key_mutex;
    bool key_valid = false;
    uint64_t key[2] = {0, 0};
};
struct maray_tape { Tape t; };

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &m) { g_err = m; return code; }

// Deeply nested expressions recurse deeply; run the recursive passes on a
// thread with a large (lazily committed) stack.
struct BigStack {
    std::function<void()> fn;
    Error err{0, ""};
    bool threw = false, bad_alloc = false;
};
void *big_stack_main(void *p)
{
    BigStack *b = (BigStack *)p;
    try { b->fn(); }
    catch (const Error &e) { b->err = e; b->threw = true; }
    catch (const std::bad_alloc &) { b->bad_alloc = true; }
    catch (const std::exception &e) { b->err = Error{MARAY_E_INTERNAL, e.what()}; b->threw = true; }
    return nullptr;
}
void run_big_stack(std::function<void()> fn)
{
    BigStack b;
    b.fn = std::move(fn);
    pthread_attr_t at;
    pthread_attr_init(&at);
    pthread_attr_setstacksize(&at, (size_t)1 << 30);
    pthread_t th;
    if (pthread_create(&th, &at, big_stack_main, &b) != 0) {
        pthread_attr_destroy(&at);
        big_stack_main(&b);
    } else {
        pthread_attr_destroy(&at);
        pthread_join(th, nullptr);
    }
    if (b.bad_alloc) throw Error{MARAY_E_INTERNAL, "out of memory"};
    if (b.threw) throw b.err;
}

template <typename F>
int guard(F f)
{
    try { f(); g_err.clear(); return MARAY_OK; }
    catch (const Error &e) { return fail(e.code, e.msg); }
    catch (const std::bad_alloc &) { return fail(MARAY_E_INTERNAL, "out of memory"); }
    catch (const std::exception &e) { return fail(MARAY_E_INTERNAL, e.what()); }
    catch (...) { return fail(MARAY_E_INTERNAL, "unknown error"); }
}

#define REQUIRE(c, what) do { if (!(c)) throw Error{MARAY_E_ARG, what}; } while (0)

// The device of every live context: what maray_hip_render_png takes its encoder for (a Backend does not say where it lives)
std::mutex g_ctx_device_mutex;
std::map<const maray_ctx *, int> &g_ctx_device = *new std::map<const maray_ctx *, int>();

}   // namespace

namespace maray {

void set_last_error(const std::string &m) { g_err = m; }

// Four independent 64-bit lanes, 32 bytes a step (a cache key, not a defence): a render call hashes its textures' bytes
// on every call -- content, not pointers: a caller may repaint a texture in place -- so the hash has to run at memory
// speed; one multiply chain per 8 bytes did 4 GB/s (1.5 ms for config 5's 6 MiB, more than the render), four chains
// side by side do ~4x that.
void hash128(const void *data, size_t n, uint64_t h[2])
{
    const unsigned char *p = (const unsigned char *)data;
    uint64_t a = h[0] ^ (n * 0x9e3779b97f4a7c15ull), b = h[1] + n, c = ~h[0] + 0x2545f4914f6cdd1dull, d = h[1] ^ 0xd6e8feb86659fd93ull;
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        memcpy(w, p + i, 32);
        a = (a ^ w[0]) * 0xff51afd7ed558ccdull; a = (a << 29) | (a >> 35);
        b = (b + w[1]) * 0xc4ceb9fe1a85ec53ull; b ^= b >> 31;
        c = (c ^ w[2]) * 0x9fb21c651e98df25ull; c = (c << 31) | (c >> 33);
        d = (d + w[3]) * 0xd6e8feb86659fd93ull; d ^= d >> 29;
    }
    for (; i + 8 <= n; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        a = (a ^ w) * 0xff51afd7ed558ccdull; a = (a << 29) | (a >> 35);
        b = (b + w) * 0xc4ceb9fe1a85ec53ull; b ^= b >> 31;
    }
    uint64_t w = 0;
    memcpy(&w, p + i, n - i);
    a = (a ^ w) * 0xff51afd7ed558ccdull; a ^= a >> 33;
    b = (b + w) * 0xc4ceb9fe1a85ec53ull; b ^= b >> 29;
    a ^= (c * 0x9e3779b97f4a7c15ull) ^ (c >> 32); b += (d * 0xff51afd7ed558ccdull) ^ (d >> 31);
    a *= 0x9e3779b97f4a7c15ull; a ^= a >> 32;
    h[0] = a * 0x9e3779b97f4a7c15ull; h[1] = b ^ a;
}

void scene_cache_key(const maray_scene *cs, uint64_t out[2])
{
    maray_scene *s = const_cast<maray_scene *>(cs);              // (the key is a cache inside the handle)
    std::lock_guard<std::mutex> lk(s->key_mutex);
    if (!s->key_valid) {
        std::vector<uint8_t> b;
        run_big_stack([&] { scene_encode(s->s, b); });
        // (the header's size is not part of a scene's program: maray_gen_to_image takes the size as arguments)
        s->key[0] = 0x6d61726179ull; s->key[1] = 3;
        hash128(b.data() + 8, b.size() >= 8 ? b.size() - 8 : 0, s->key);
        s->key_valid = true;
    }
    out[0] = s->key[0]; out[1] = s->key[1];
    // Declared parameters are not in the encoding but they are part of the program (its ranges, which Var ids are operands):
    // folded in here, on every read, so that whatever renamed or dropped the scene's own name above -- rescale, supersample,
    // simplify, ... -- keeps them.  Values are not part of the name: every frame of an animation finds the same program.
    for (const ParamDecl &pd : s->s.params) {
        struct { uint64_t tag, id; double lo, hi; } d = {0x5041524Dull, pd.id, pd.lo, pd.hi};      // "PARM"
        hash128(&d, sizeof d, out);
    }
}

// gen_to_image with samples = k: a private copy of the scene, supersampled (named after the scene and k)
maray_scene *scene_supersampled_copy(const maray_scene *cs, uint32_t k)
{
    std::unique_ptr<maray_scene> c(new maray_scene());
    {
        maray_scene *s = const_cast<maray_scene *>(cs);
        std::lock_guard<std::mutex> lk(s->key_mutex);
        c->s = s->s;
        c->key_valid = s->key_valid; c->key[0] = s->key[0]; c->key[1] = s->key[1];
    }
    if (const int rc = maray_scene_supersample(c.get(), k)) throw Error{rc, maray_last_error()};
    return c.release();
}

maray_program load_program(const maray_program *p)
{
    if (!p) throw Error{MARAY_E_ARG, "null argument"};
    maray_program r;
    memset(&r, 0, sizeof r);
    memcpy(&r, p, offsetof(maray_program, n_params));        // what a version-2 struct has
    if (p->version == MARAY_TAPE_VERSION_PARAMS) { r.n_params = p->n_params; r.param_ranges = p->param_ranges; }
    return r;
}

bool param_value_ok(const double *ranges, uint32_t p, double v)
{
    const double lo = ranges[2 * p], hi = ranges[2 * p + 1];
    if (lo == -INFINITY && hi == INFINITY) return true;          // anything, NaN included
    if (!(v >= lo && v <= hi)) return false;                     // (false for NaN)
    if (v == 0.0 && lo == 0.0 && std::signbit(v) && !std::signbit(lo)) return false;      // -0.0 is below +0.0 here
    if (v == 0.0 && hi == 0.0 && !std::signbit(v) && std::signbit(hi)) return false;
    return true;
}

void validate_program(const maray_program &p)
{
    if (p.version != MARAY_TAPE_VERSION && p.version != MARAY_TAPE_VERSION_PARAMS) throw Error{MARAY_E_ARG, "tape version mismatch"};
    const uint32_t n_params = p.version == MARAY_TAPE_VERSION_PARAMS ? p.n_params : 0u;
    if (p.version == MARAY_TAPE_VERSION_PARAMS) {
        if (n_params == 0 || n_params > MARAY_MAX_PARAMS || !p.param_ranges) throw Error{MARAY_E_ARG, "a version-3 program has 1 to 64 parameters and their ranges"};
        for (uint32_t k = 0; k < n_params; k++)
            if (!(p.param_ranges[2 * k] <= p.param_ranges[2 * k + 1])) throw Error{MARAY_E_ARG, "parameter range with lo > hi or a NaN bound"};
    }
    if ((p.n_consts && !p.consts) || (p.n_row_ops && !p.row_ops) || (p.n_pix_ops && !p.pix_ops))
        throw Error{MARAY_E_ARG, "null section pointer"};
    if (p.n_row_slots > MARAY_MAX_SLOTS || p.n_pix_slots > MARAY_MAX_SLOTS) throw Error{MARAY_E_LIMIT, "too many slots"};
    const uint32_t n_ynum = numeric_yvals(p);       // y values past these only gate SKIP ops (guards)
    auto check = [&](const uint64_t *ops, uint32_t n, uint32_t n_slots, bool pixel) {
        std::vector<uint8_t> written(n_slots, 0);
        bool have_acc = false;
        struct Region { uint32_t end; std::vector<uint8_t> before; uint32_t dst; };
        std::vector<Region> regions;               // open SKIPZ / SKIPNZ regions, innermost last
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t ins = ops[i];
            const uint32_t op = MARAY_INS_OP(ins), aux = MARAY_INS_AUX(ins), dst = MARAY_INS_DST(ins);
            if (op >= MARAY_OP_COUNT) throw Error{MARAY_E_ARG, "invalid opcode at op " + std::to_string(i)};
            auto close_regions = [&]() {
                // values written only inside a skipped region do not exist on the skip path
                while (!regions.empty() && regions.back().end == i) {
                    written = regions.back().before;
                    if (regions.back().dst != MARAY_DST_NONE) written[regions.back().dst] = 1;
                    if (dst != regions.back().dst) throw Error{MARAY_E_ARG, "skip region does not end in its own destination at op " + std::to_string(i)};
                    regions.pop_back();
                }
            };
            if (op == MARAY_OP_NOP) { close_regions(); continue; }
            const int arity = (op == MARAY_OP_TEXDIM) ? 0 : (op >= MARAY_OP_ADD && op <= MARAY_OP_APP) ? 2 : 1;   // STEPSIN, OUT, MOV, SKIP* and the unary ops read `a` only
            const uint32_t refs[2] = {MARAY_INS_A(ins), MARAY_INS_B(ins)};
            for (int k = 0; k < arity; k++) {
                const uint32_t kind = MARAY_REF_KIND(refs[k]), idx = MARAY_REF_INDEX(refs[k]);
                bool ok = true;
                switch (kind) {
                case MARAY_K_SLOT: ok = idx < n_slots && written[idx]; break;
                case MARAY_K_CONST: ok = idx < p.n_consts; break;
                case MARAY_K_YVAL: ok = pixel && idx < p.n_yvals; break;
                default: ok = idx >= MARAY_SPEC_PARAM0 ? idx - MARAY_SPEC_PARAM0 < n_params :      // a parameter: either section
                              (idx != MARAY_SPEC_ACC || have_acc) && (idx != MARAY_SPEC_X || pixel) &&
                              (idx < MARAY_SPEC_XMAX || !pixel);      // the span specials are for the ROW section
                }
                if (!ok) throw Error{MARAY_E_ARG, "operand out of range or read before write at op " + std::to_string(i)};
            }
            if (op == MARAY_OP_OUT) {
                if (aux >= (pixel ? 3u : p.n_yvals)) throw Error{MARAY_E_ARG, "output index out of range at op " + std::to_string(i)};
                if (!regions.empty()) throw Error{MARAY_E_ARG, "OUT inside a skip region at op " + std::to_string(i)};
                continue;
            }
            if (op == MARAY_OP_SKIPZ || op == MARAY_OP_SKIPNZ) {
                if (aux == 0 || (uint64_t)i + aux >= n) throw Error{MARAY_E_ARG, "skip count out of range at op " + std::to_string(i)};
                if (!regions.empty() && i + aux > regions.back().end) throw Error{MARAY_E_ARG, "skip regions overlap at op " + std::to_string(i)};
                if (dst != MARAY_DST_NONE && dst >= n_slots) throw Error{MARAY_E_ARG, "dst slot out of range at op " + std::to_string(i)};
                // a guard (a y value nothing reads as an operand) is a bound, "0 => the boolean is 0 over the span": the
                // evaluators keep it as one bit (!= 0) or do not keep its value at all; it can gate a SKIPZ only
                if (op == MARAY_OP_SKIPNZ && MARAY_REF_KIND(refs[0]) == MARAY_K_YVAL && MARAY_REF_INDEX(refs[0]) >= n_ynum)
                    throw Error{MARAY_E_ARG, "SKIPNZ on a guard y value at op " + std::to_string(i) + " (guards gate SKIPZ only)"};
                const uint32_t last = MARAY_INS_OP(ops[i + aux]);
                if (!(last == MARAY_OP_MUL || last == MARAY_OP_MIN || last == MARAY_OP_MAX))
                    throw Error{MARAY_E_ARG, "skip region must end in Mul / Min / Max at op " + std::to_string(i)};
                regions.push_back(Region{i + aux, written, dst});
                continue;
            }
            if ((op == MARAY_OP_APP || op == MARAY_OP_TEXDIM) && aux >= p.n_app)
                throw Error{MARAY_E_ARG, "App id above n_app at op " + std::to_string(i)};
            if (dst != MARAY_DST_NONE) {
                if (dst >= n_slots) throw Error{MARAY_E_ARG, "dst slot out of range at op " + std::to_string(i)};
                written[dst] = 1;
            }
            have_acc = true;
            close_regions();
        }
        if (!regions.empty()) throw Error{MARAY_E_ARG, "unterminated skip region"};
    };
    check(p.row_ops, p.n_row_ops, p.n_row_slots, false);
    check(p.pix_ops, p.n_pix_ops, p.n_pix_slots, true);
}

// A REFINE section handed in beside a program: the ROW section's checks (no X, no YVAL), no Y either, and every OUT names a
// guard of the program.
void validate_refine(const maray_program &p, const maray_refine &r)
{
    if (!r.ops || (r.n_consts && !r.consts)) throw Error{MARAY_E_ARG, "null section pointer"};
    maray_program q = p;
    q.n_consts = r.n_consts; q.consts = r.consts;
    q.n_row_ops = r.n_ops; q.row_ops = r.ops; q.n_row_slots = r.n_slots;
    q.n_pix_ops = 0; q.pix_ops = nullptr;           // (the PIXEL section reads the program's own constant pool)
    validate_program(q);
    const uint32_t n_ynum = numeric_yvals(p);
    for (uint32_t i = 0; i < r.n_ops; i++) {
        const uint64_t ins = r.ops[i];
        const uint32_t op = MARAY_INS_OP(ins);
        if (op == MARAY_OP_NOP || op == MARAY_OP_TEXDIM) continue;
        if (op == MARAY_OP_OUT && MARAY_INS_AUX(ins) < n_ynum) throw Error{MARAY_E_ARG, "REFINE output " + std::to_string(MARAY_INS_AUX(ins)) + " is not a guard"};
        const uint32_t refs[2] = {MARAY_INS_A(ins), (op >= MARAY_OP_ADD && op <= MARAY_OP_APP) ? MARAY_INS_B(ins) : 0u};
        for (uint32_t ref : refs)
            if (MARAY_REF_KIND(ref) == MARAY_K_SPEC && MARAY_REF_INDEX(ref) == MARAY_SPEC_Y) throw Error{MARAY_E_ARG, "the REFINE section reads Y at op " + std::to_string(i)};
    }
}

}   // namespace maray

extern "C" {

const char *maray_last_error(void) { return g_err.c_str(); }
const char *maray_version(void) { return "maray_amd 0.1 (gfx950; tape v2; mirrors maray 0.3.8)"; }

// ---- scenes ------------------------------------------------------------------
static void name_from_bytes(maray_scene *s, const uint8_t *buf, size_t len)
{
    std::lock_guard<std::mutex> lk(s->key_mutex);
    s->key[0] = 0x6d61726179ull; s->key[1] = 3;
    hash128(buf + (len >= 8 ? 8 : len), len >= 8 ? len - 8 : 0, s->key);
    s->key_valid = true;
}

int maray_scene_from_bytes(const uint8_t *buf, size_t len, maray_scene **out)
{
    return guard([&] {
        REQUIRE(buf && out, "null argument");
        *out = nullptr;
        maray_scene *s = new maray_scene();
        try { run_big_stack([&] { scene_decode(buf, len, s->s); }); }
        catch (...) { delete s; throw; }
        name_from_bytes(s, buf, len);
        *out = s;
    });
}

int maray_scene_open(const char *path, maray_scene **out)
{
    return guard([&] {
        REQUIRE(path && out, "null argument");
        *out = nullptr;
        FILE *f = fopen(path, "rb");
        if (!f) throw Error{MARAY_E_IO, std::string("cannot open ") + path};
        std::vector<uint8_t> b;
        uint8_t tmp[65536];
        size_t n;
        while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) b.insert(b.end(), tmp, tmp + n);
        fclose(f);
        maray_scene *s = new maray_scene();
        try { run_big_stack([&] { scene_decode(b.data(), b.size(), s->s); }); }
        catch (...) { delete s; throw; }
        name_from_bytes(s, b.data(), b.size());
        *out = s;
    });
}

void maray_scene_free(maray_scene *s) { delete s; }

int maray_scene_size(const maray_scene *s, uint32_t *w, uint32_t *h)
{
    return guard([&] { REQUIRE(s && w && h, "null argument"); *w = s->s.w; *h = s->s.h; });
}

int maray_scene_set_size(maray_scene *s, uint32_t w, uint32_t h)
{
    return guard([&] { REQUIRE(s, "null argument"); s->key_valid = false; s->s.w = w; s->s.h = h; });
}

int maray_scene_is_legacy(const maray_scene *s, int *legacy)
{
    return guard([&] { REQUIRE(s && legacy, "null argument"); *legacy = s->s.legacy ? 1 : 0; });
}

int maray_scene_node_count(const maray_scene *s, int c, uint64_t *n)
{
    return guard([&] {
        REQUIRE(s && n && c >= 0 && c < 3, "bad argument");
        run_big_stack([&] { *n = scene_node_count(s->s, c); });
    });
}

int maray_scene_encode(const maray_scene *s, uint8_t *out, size_t cap, size_t *len_out)
{
    return guard([&] {
        REQUIRE(s && len_out, "null argument");
        std::vector<uint8_t> b;
        run_big_stack([&] { scene_encode(s->s, b); });
        *len_out = b.size();
        if (out && cap >= b.size()) memcpy(out, b.data(), b.size());
    });
}

int maray_scene_save(const maray_scene *s, const char *path)
{
    return guard([&] {
        REQUIRE(s && path, "null argument");
        std::vector<uint8_t> b;
        run_big_stack([&] { scene_encode(s->s, b); });
        FILE *f = fopen(path, "wb");
        if (!f) throw Error{MARAY_E_IO, std::string("cannot create ") + path};
        size_t n = fwrite(b.data(), 1, b.size(), f);
        fclose(f);
        if (n != b.size()) throw Error{MARAY_E_IO, "short write"};
    });
}

int maray_scene_fix_color(maray_scene *s)
{
    return guard([&] { REQUIRE(s, "null argument"); s->key_valid = false; run_big_stack([&] { scene_fix_color(s->s); }); });
}

int maray_scene_rescale(maray_scene *s, uint32_t sx, uint32_t sy)
{
    return guard([&] {
        REQUIRE(s, "null argument");
        // the name is dropped while the scene changes and folded forward only once the rescale has succeeded: a rescale that
        // throws must not leave a name that a cached tape of another program answers to
        bool named;
        {
            std::lock_guard<std::mutex> lk(s->key_mutex);
            named = s->key_valid;
            s->key_valid = false;
        }
        scene_rescale(s->s, sx, sy);
        std::lock_guard<std::mutex> lk(s->key_mutex);
        if (named) { const uint32_t step[3] = {0x52455343u, sx, sy}; hash128(step, sizeof step, s->key); s->key_valid = true; }      // "RESC", factors
    });
}

int maray_scene_supersample(maray_scene *s, uint32_t k)
{
    return guard([&] {
        REQUIRE(s, "null argument");
        if (k == 0) k = 1;
        bool named;         // dropped while the scene changes, folded forward after success (as in maray_scene_rescale)
        {
            std::lock_guard<std::mutex> lk(s->key_mutex);
            named = s->key_valid;
            s->key_valid = false;
        }
        try { scene_supersample(s->s, k); }
        catch (...) { std::lock_guard<std::mutex> lk(s->key_mutex); s->key_valid = named; throw; }     // unchanged: so is its name
        std::lock_guard<std::mutex> lk(s->key_mutex);
        if (named && k > 1) { const uint32_t step[2] = {0x53555053u, k}; hash128(step, sizeof step, s->key); }      // "SUPS", k
        s->key_valid = named;
    });
}

// ---- scene parameters ---------------------------------------------------------
uint64_t maray_var_id(const char *name)
{
    // `var(name)` (src/lib.rs:845-850): fnv::FnvHasher (FNV-1a, 64 bits) over what Rust's `str::hash` feeds it, the name's
    // bytes and a 0xff terminator; the same id as var() of include/maray_builders.hpp
    uint64_t h = 0xcbf29ce484222325ull;
    for (const unsigned char *p = (const unsigned char *)(name ? name : ""); *p; p++) { h ^= *p; h *= 0x100000001b3ull; }
    h ^= 0xffu; h *= 0x100000001b3ull;
    return h;
}

int maray_scene_declare_param(maray_scene *s, uint64_t var_id, double lo, double hi, uint32_t *index)
{
    return guard([&] {
        REQUIRE(s, "null argument");
        REQUIRE(lo <= hi, "parameter range with lo > hi or a NaN bound");
        std::vector<ParamDecl> &ps = s->s.params;
        for (size_t k = 0; k < ps.size(); k++)
            if (ps[k].id == var_id) {
                REQUIRE(memcmp(&ps[k].lo, &lo, 8) == 0 && memcmp(&ps[k].hi, &hi, 8) == 0, "parameter declared twice with different ranges");
                if (index) *index = (uint32_t)k;
                return;
            }
        if (ps.size() >= MARAY_MAX_PARAMS) throw Error{MARAY_E_LIMIT, "more than 64 parameters"};
        ParamDecl pd;
        pd.id = var_id; pd.lo = lo; pd.hi = hi; pd.value = NAN;
        // (the scene's stored name does not change: declarations are folded into it where it is read, scene_cache_key)
        std::lock_guard<std::mutex> lk(s->key_mutex);
        ps.push_back(pd);
        if (index) *index = (uint32_t)ps.size() - 1;
    });
}

int maray_scene_param_count(const maray_scene *s, uint32_t *n)
{
    return guard([&] { REQUIRE(s && n, "null argument"); *n = (uint32_t)s->s.params.size(); });
}

int maray_scene_param_info(const maray_scene *s, uint32_t index, uint64_t *var_id, double *lo, double *hi, double *value)
{
    return guard([&] {
        REQUIRE(s && index < s->s.params.size(), "no such parameter");
        const ParamDecl &pd = s->s.params[index];
        if (var_id) *var_id = pd.id;
        if (lo) *lo = pd.lo;
        if (hi) *hi = pd.hi;
        if (value) *value = pd.value;
    });
}

int maray_scene_set_param(maray_scene *s, uint32_t index, double value)
{
    return guard([&] {
        REQUIRE(s && index < s->s.params.size(), "no such parameter");
        ParamDecl &pd = s->s.params[index];
        const double r[2] = {pd.lo, pd.hi};
        REQUIRE(param_value_ok(r, 0, value), "parameter value outside its declared range");
        pd.value = value;
    });
}

// ---- shutter: the scene layer (host only) -------------------------------------------
int maray_scene_set_param_span(maray_scene *s, uint32_t index, double span)
{
    return guard([&] {
        REQUIRE(s && index < s->s.params.size(), "no such parameter");
        REQUIRE(span >= 0.0 && std::isfinite(span), "a parameter's span is finite and >= 0");
        s->s.params[index].span = span;
    });
}

int maray_scene_param_span(const maray_scene *s, uint32_t index, double *span)
{
    return guard([&] {
        REQUIRE(s && span && index < s->s.params.size(), "no such parameter");
        *span = s->s.params[index].span;
    });
}

int maray_scene_shutter_values(const maray_scene *s, uint32_t n, double *out)
{
    return guard([&] {
        REQUIRE(s, "null argument");
        REQUIRE(shutter_frames_ok(n), "shutter frames must be 1, 2, 4, 8, 16, 32 or 64");
        const size_t P = s->s.params.size();
        REQUIRE(out || !P, "null argument");
        for (uint32_t i = 0; i < n; i++) {
            // exact: |2i + 1 - n| < 64 over a power of two
            const double c = (double)(2 * (int)i + 1 - (int)n) / (double)(2 * (int)n);
            for (size_t p = 0; p < P; p++) {
                const ParamDecl &pd = s->s.params[p];
                double v = pd.value;            // span 0: the value itself, bit for bit (-0.0 and NaN stay what they are)
                if (pd.span > 0.0) {
                    const double step = pd.span * c;     // one multiply, one add, never fused (-ffp-contract=off)
                    v = pd.value + step;
                }
                out[(size_t)i * P + p] = v;
            }
        }
    });
}

int maray_scene_simplify(maray_scene *s)
{
    return guard([&] { REQUIRE(s, "null argument"); s->key_valid = false; run_big_stack([&] { scene_simplify(s->s); }); });
}

int maray_scene_simplify_ex(maray_scene *s, uint32_t flags)
{
    return guard([&] {
        REQUIRE(s, "null argument"); s->key_valid = false;
        REQUIRE((flags & ~(uint32_t)MARAY_SIMPLIFY_MERGE_DIVISORS) == 0, "unknown simplify flag");
        run_big_stack([&] { scene_simplify(s->s, flags); });
    });
}

int maray_scene_compress(maray_scene *s, uint32_t *n_vars3)
{
    return guard([&] { REQUIRE(s, "null argument"); s->key_valid = false; run_big_stack([&] { scene_compress(s->s, n_vars3); }); });
}

int maray_scene_display_len(maray_scene *s, int c, uint64_t *len)
{
    return guard([&] {
        REQUIRE(s && len && c >= 0 && c < 3, "bad argument"); s->key_valid = false;
        run_big_stack([&] { *len = scene_display_len(s->s, c); });
    });
}

// ---- lowering -----------------------------------------------------------------
int maray_lower(const maray_scene *s, const maray_lower_opts *opts, maray_tape **out)
{
    return guard([&] {
        REQUIRE(s && out, "null argument");
        *out = nullptr;
        maray_lower_opts o;
        memset(&o, 0, sizeof o);
        o.hoist_rows = 1;
        if (opts) o = *opts;
        maray_tape *t = new maray_tape();
        try {
            run_big_stack([&] { lower_scene(s->s, o, t->t); });
            validate_program(t->t.program());
        } catch (...) { delete t; throw; }
        *out = t;
    });
}

void maray_tape_free(maray_tape *t) { delete t; }

int maray_tape_program(const maray_tape *t, maray_program *out)
{
    return guard([&] { REQUIRE(t && out, "null argument"); *out = t->t.program(); });
}

int maray_tape_get_info(const maray_tape *t, maray_tape_info *out)
{
    return guard([&] { REQUIRE(t && out, "null argument"); *out = t->t.info; });
}

int maray_tape_param_count(const maray_tape *t, uint32_t *n)
{
    return guard([&] { REQUIRE(t && n, "null argument"); *n = (uint32_t)(t->t.param_ranges.size() / 2); });
}

int maray_tape_param_range(const maray_tape *t, uint32_t index, double *lo, double *hi)
{
    return guard([&] {
        REQUIRE(t && lo && hi && index < t->t.param_ranges.size() / 2, "no such parameter");
        *lo = t->t.param_ranges[2 * index]; *hi = t->t.param_ranges[2 * index + 1];
    });
}

int maray_tape_refine(const maray_tape *t, maray_refine *out)
{
    return guard([&] { REQUIRE(t && out, "null argument"); *out = t->t.refine(); });
}

// ---- device ---------------------------------------------------------------------
int maray_hip_device_count(int *n)
{
    return guard([&] { REQUIRE(n, "null argument"); *n = hip_device_count(); });
}

int maray_hip_ctx_create(int device, const maray_program *prog, const maray_texture *tex, uint32_t n_tex,
                         const maray_ctx_opts *opts, maray_ctx **out)
{
    return maray_hip_ctx_create_refined(device, prog, nullptr, tex, n_tex, opts, out);
}

int maray_hip_ctx_create_refined(int device, const maray_program *prog, const maray_refine *refine, const maray_texture *tex, uint32_t n_tex,
                                 const maray_ctx_opts *opts, maray_ctx **out)
{
    return guard([&] {
        REQUIRE(prog && out, "null argument");
        REQUIRE(n_tex == 0 || tex, "null texture table");
        *out = nullptr;
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        validate_program(*prog);
        if (refine && !refine->n_ops) refine = nullptr;
        if (refine) validate_refine(*prog, *refine);
        if (prog->n_app > 5u * n_tex)   // reference: rt.functions[id] panics (src/lib.rs:665)
            throw Error{MARAY_E_APP_RANGE, "scene calls App id " + std::to_string(prog->n_app - 1) + " but only " +
                        std::to_string(5u * n_tex) + " texture functions exist"};
        for (uint32_t i = 0; i < n_tex; i++) REQUIRE(tex[i].rgb || (uint64_t)tex[i].w * tex[i].h == 0, "null texture raster");
        const uint32_t backend = opts ? opts->backend : MARAY_BACKEND_TAPE;
        uint32_t samples = opts && opts->samples ? opts->samples : 1u;
        REQUIRE(samples == 1 || samples == 2 || samples == 4 || samples == 8, "samples must be 0, 1, 2, 4 or 8");
        const uint32_t filter = opts ? opts->filter : (uint32_t)MARAY_FILTER_BOX;
        REQUIRE(filter == MARAY_FILTER_BOX || filter == MARAY_FILTER_TENT || filter == MARAY_FILTER_CATROM, "unknown filter");
        REQUIRE(filter != MARAY_FILTER_TENT || samples > 1, "the tent filter needs samples = 2, 4 or 8");
        REQUIRE(filter != MARAY_FILTER_CATROM || samples > 1, "the Catmull-Rom filter needs samples = 2, 4 or 8");
        const uint32_t transfer = opts ? opts->transfer : (uint32_t)MARAY_TRANSFER_NONE;
        REQUIRE(transfer == MARAY_TRANSFER_NONE || transfer == MARAY_TRANSFER_SRGB, "unknown transfer");
        REQUIRE(filter != MARAY_FILTER_CATROM || transfer == MARAY_TRANSFER_NONE, "the Catmull-Rom filter in linear light (MARAY_TRANSFER_SRGB) is not built");
        // a tent or Catmull-Rom context is a plain back-end of the (supersampled) program behind the filter's wrapper (filter_backend.cpp); so
        // is every MARAY_TRANSFER_SRGB context: its box reduce is a kernel of the wrapper's, not the in-kernel one
        const uint32_t k = samples;
        const bool wrapped = filter == MARAY_FILTER_TENT || filter == MARAY_FILTER_CATROM || transfer == MARAY_TRANSFER_SRGB;
        if (wrapped) samples = 1;
        Backend *b = nullptr;
        switch (backend) {
        case MARAY_BACKEND_TAPE: b = make_tape_backend(device, *prog, tex, n_tex, true, samples); break;
        case MARAY_BACKEND_TAPE_SMEM: b = make_tape_backend(device, *prog, tex, n_tex, false, samples); break;
        case MARAY_BACKEND_JIT: b = make_jit_backend(device, *prog, tex, n_tex, samples, refine); break;
        case MARAY_BACKEND_AUTO: {
            // One-shot economics.  The specialised kernels render a frame tens of times faster than the interpreter, but
            // hiprtc needs seconds to build them (chess: 9 k pixel + 17 k row ops -> 1.6 s with the two modules built side
            // by side; 1,000 triangles, 36 k + 37 k ops -> 15-20 s; before the lowering privatised shared values a 49 k-op
            // scene took 6.5 min), the interpreter needs none.  So: take them when the code objects are already in the cache, or when the
            // caller says how much it will render (hint_mpixels) and the interpreter would need longer for that than
            // the build takes, or when it does not say (a context kept for many frames).  Estimates, measured on chess
            // and the triangle soups: build 0.5 s + 0.4 ms per pixel op + 0.24 ms per row op;
            // interpreter 4.4 us per megapixel and executed op, of which guards skip ~95 % when the program has any.
            const char *force = getenv("MARAY_AUTO");          // "jit" / "tape": override (measurements)
            bool want_jit = prog->n_pix_ops <= 25000;
            if (want_jit && opts && opts->hint_mpixels) {
                // cached code objects cost a context ~0.02 s more than the interpreter's (two module loads; the key comes from the
                // program's name, jit_build.cpp) -- 0.2 s when the process has to generate the sources for the key first
                const double build_s = jit_code_is_cached(*prog) ? 0.02 : 0.5 + 4.0e-4 * prog->n_pix_ops + 2.4e-4 * prog->n_row_ops;
                const bool guarded = prog->n_yvals > numeric_yvals(*prog);
                const double interp_s = (double)opts->hint_mpixels * prog->n_pix_ops * 4.4e-6 * (guarded ? 0.05 : 1.0);
                want_jit = interp_s > build_s;
            }
            if (force && !strcmp(force, "jit")) want_jit = true;
            if (force && !strcmp(force, "tape")) want_jit = false;
            if (!want_jit) { b = make_tape_backend(device, *prog, tex, n_tex, false, samples); break; }
            try { b = make_jit_backend(device, *prog, tex, n_tex, samples, refine); }
            catch (const Error &e) {
                if (e.code == MARAY_E_NO_DEVICE) throw;
                b = make_tape_backend(device, *prog, tex, n_tex, false, samples);   // still the HIP path, never a CPU fallback
            }
            break;
        }
        default: throw Error{MARAY_E_ARG, "unknown backend"};
        }
        if (wrapped) {
            try { b = make_filter_backend(device, b, k, prog->n_params, filter, transfer); }
            catch (...) { delete b; throw; }
        }
        maray_ctx *c = new maray_ctx();
        c->backend = b;
        c->n_tex = n_tex;
        c->samples = k;             // (a tent context too takes output geometry, RGB8 only, k w and k h within the domain)
        if (prog->n_params) c->param_ranges.assign(prog->param_ranges, prog->param_ranges + 2 * (size_t)prog->n_params);
        for (uint32_t p = 0; p < prog->n_params; p++) c->params_ready = c->params_ready && param_value_ok(c->param_ranges.data(), p, NAN);
        { std::lock_guard<std::mutex> lk(g_ctx_device_mutex); g_ctx_device[c] = device; }
        *out = c;
    });
}

int maray_hip_ctx_param_count(const maray_ctx *c, uint32_t *n)
{
    return guard([&] { REQUIRE(c && n, "null argument"); *n = (uint32_t)(c->param_ranges.size() / 2); });
}

int maray_hip_ctx_set_params(maray_ctx *c, const double *values, uint32_t n)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        REQUIRE(n == c->param_ranges.size() / 2, "parameter count differs from the program's");
        if (!n) return;
        REQUIRE(values, "null argument");
        // every value is checked before any is taken: a call that fails leaves the old values.  The ranges are the program's:
        // what the lowering proved -- a bounded Sin's table index among it -- holds for values inside them only.
        for (uint32_t p = 0; p < n; p++)
            if (!param_value_ok(c->param_ranges.data(), p, values[p]))
                throw Error{MARAY_E_ARG, "value of parameter " + std::to_string(p) + " is outside its declared range"};
        c->backend->set_params(values, n);
        c->params_ready = true;
    });
}

void maray_hip_ctx_free(maray_ctx *c)
{
    if (!c) return;
    { std::lock_guard<std::mutex> lk(g_ctx_device_mutex); g_ctx_device.erase(c); }
    delete c->backend;
    delete c;
}

static void check_rows(uint32_t w, uint32_t h, uint32_t y0, uint32_t y1)
{
    if (y0 > y1 || y1 > h) throw Error{MARAY_E_ARG, "row range out of bounds"};
    // the lowering's interval analysis (bounded Sin arguments, row bounds) covers x, y < MARAY_DOMAIN_MAX
    if (w > MARAY_DOMAIN_MAX || y1 > MARAY_DOMAIN_MAX)
        throw Error{MARAY_E_LIMIT, "image exceeds " + std::to_string(MARAY_DOMAIN_MAX) + " pixels in x or y"};
}

// A supersampling context evaluates k w x k h samples: the lowering's analysis covers sample indices below
// MARAY_DOMAIN_MAX.  It writes RGB8 only.
static void check_samples(const maray_ctx *c, uint32_t w, uint32_t h, bool want64, bool own_values = false)
{
    if (!c->params_ready && !own_values) throw Error{MARAY_E_ARG, "the program's parameters have ranges that exclude NaN and no values yet: call maray_hip_ctx_set_params first"};
    if (c->samples <= 1) return;
    if (want64) throw Error{MARAY_E_ARG, "a supersampling context renders RGB8 only (no f64 planes)"};
    if ((uint64_t)w * c->samples > MARAY_DOMAIN_MAX || (uint64_t)h * c->samples > MARAY_DOMAIN_MAX)
        throw Error{MARAY_E_LIMIT, "supersampled image exceeds " + std::to_string(MARAY_DOMAIN_MAX) + " samples in x or y"};
}

int maray_hip_render_rows(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, uint8_t *rgb8, double *rgb64)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        check_rows(w, h, y0, y1);
        check_samples(c, w, h, rgb64 != nullptr);
        if (y0 == y1 || w == 0 || (!rgb8 && !rgb64)) return;
        c->backend->render_host_tiles(w, h, cut_row_tiles(w, y0, y1, rgb8 != nullptr, rgb64 != nullptr), y0, rgb8, rgb64, nullptr);
    });
}

int maray_hip_render_tiles(maray_ctx *c, uint32_t w, uint32_t h, const uint32_t *tiles_y0y1, uint32_t n_tiles,
                           uint8_t *rgb8_image, maray_tile_fn fn, void *user)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        REQUIRE(n_tiles == 0 || tiles_y0y1, "null tile list");
        if (n_tiles == 0 || w == 0 || !rgb8_image) return;
        std::vector<RowTile> tiles(n_tiles);
        for (uint32_t i = 0; i < n_tiles; i++) {
            tiles[i] = RowTile{tiles_y0y1[2 * i], tiles_y0y1[2 * i + 1]};
            check_rows(w, h, tiles[i].y0, tiles[i].y1);
            REQUIRE(tiles[i].y1 > tiles[i].y0, "empty tile");
        }
        check_samples(c, w, h, false);
        std::function<void(uint32_t, uint32_t)> done;
        if (fn) done = [&](uint32_t a, uint32_t b) { fn(user, a, b); };
        c->backend->render_host_tiles(w, h, tiles, 0, rgb8_image, nullptr, done);
    });
}

// ---- shutter ------------------------------------------------------------------------
// n and every value of every frame, before anything is enqueued: one bad value and the call has done nothing
static void check_shutter(const maray_ctx *c, const double *values, uint32_t n)
{
    REQUIRE(shutter_frames_ok(n), "shutter frames must be 1, 2, 4, 8, 16, 32 or 64");
    const uint32_t P = (uint32_t)(c->param_ranges.size() / 2);
    if (!P) return;
    REQUIRE(values, "null argument: a program with parameters needs the frames' values");
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t p = 0; p < P; p++)
            if (!param_value_ok(c->param_ranges.data(), p, values[(size_t)i * P + p]))
                throw Error{MARAY_E_ARG, "frame " + std::to_string(i) + ": value of parameter " + std::to_string(p) + " is outside its declared range"};
}

int maray_hip_render_rows_shutter(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, const double *values, uint32_t n, uint8_t *rgb8)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        check_rows(w, h, y0, y1);
        check_samples(c, w, h, false, true);
        check_shutter(c, values, n);
        if (y0 == y1 || w == 0 || !rgb8) return;
        c->backend->render_host_tiles_shutter(w, h, cut_row_tiles(w, y0, y1, true, false), y0, values, n, rgb8, nullptr);
    });
}

int maray_hip_render_rows_shutter_device(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1, const double *values, uint32_t n,
                                         void *d_rgb8, void *stream)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        check_rows(w, h, y0, y1);
        check_samples(c, w, h, false, true);
        check_shutter(c, values, n);
        if (y0 == y1 || w == 0) return;
        REQUIRE(d_rgb8, "null argument");
        c->backend->render_device_shutter(w, h, RowBlocks::range(y0, y1), values, n, d_rgb8, stream);
    });
}

int maray_hip_render_tiles_shutter(maray_ctx *c, uint32_t w, uint32_t h, const uint32_t *tiles_y0y1, uint32_t n_tiles, const double *values, uint32_t n,
                                   uint8_t *rgb8_image, maray_tile_fn fn, void *user)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        REQUIRE(n_tiles == 0 || tiles_y0y1, "null tile list");
        std::vector<RowTile> tiles(n_tiles);
        for (uint32_t i = 0; i < n_tiles; i++) {
            tiles[i] = RowTile{tiles_y0y1[2 * i], tiles_y0y1[2 * i + 1]};
            check_rows(w, h, tiles[i].y0, tiles[i].y1);
            REQUIRE(tiles[i].y1 > tiles[i].y0, "empty tile");
        }
        check_samples(c, w, h, false, true);
        check_shutter(c, values, n);
        if (n_tiles == 0 || w == 0 || !rgb8_image) return;
        std::function<void(uint32_t, uint32_t)> done;
        if (fn) done = [&](uint32_t a, uint32_t b) { fn(user, a, b); };
        c->backend->render_host_tiles_shutter(w, h, tiles, 0, values, n, rgb8_image, done);
    });
}

int maray_hip_time_shutter_reduce(int device, size_t bytes, uint32_t n, int reps, float *ms_avg)
{
    return guard([&] {
        REQUIRE(ms_avg, "null argument");
        *ms_avg = shutter_time_reduce(device, bytes, n, reps);
    });
}

int maray_hip_time_filter(int device, uint32_t w, uint32_t rows, uint32_t k, int reps, float *ms_avg)
{
    return guard([&] {
        REQUIRE(ms_avg, "null argument");
        *ms_avg = filter_time_tent(device, w, rows, k, reps);
    });
}

int maray_hip_time_filter_ex(int device, uint32_t w, uint32_t rows, uint32_t k, uint32_t filter, uint32_t transfer, int reps, float *ms_avg)
{
    return guard([&] {
        REQUIRE(ms_avg, "null argument");
        REQUIRE(filter == MARAY_FILTER_BOX || filter == MARAY_FILTER_TENT || filter == MARAY_FILTER_CATROM, "unknown filter");
        REQUIRE(transfer == MARAY_TRANSFER_NONE || transfer == MARAY_TRANSFER_SRGB, "unknown transfer");
        REQUIRE(filter != MARAY_FILTER_CATROM || transfer == MARAY_TRANSFER_NONE, "the Catmull-Rom filter in linear light (MARAY_TRANSFER_SRGB) is not built");
        REQUIRE(filter != MARAY_FILTER_BOX || transfer == MARAY_TRANSFER_SRGB, "the plain box reduce has no kernel of its own");
        *ms_avg = transfer == MARAY_TRANSFER_SRGB ? filter_time_lin(device, w, rows, k, filter, reps)
                : filter == MARAY_FILTER_CATROM   ? filter_time_catrom(device, w, rows, k, reps)
                                                  : filter_time_tent(device, w, rows, k, reps);
    });
}

int maray_hip_time_shutter_reduce_ex(int device, size_t bytes, uint32_t n, uint32_t transfer, int reps, float *ms_avg)
{
    return guard([&] {
        REQUIRE(ms_avg, "null argument");
        REQUIRE(transfer == MARAY_TRANSFER_NONE || transfer == MARAY_TRANSFER_SRGB, "unknown transfer");
        *ms_avg = shutter_time_reduce(device, bytes, n, reps, transfer);
    });
}

// ---- transfer (include/maray_hip.h) ----------------------------------------------------------------------------------
int maray_transfer_table(uint32_t transfer, uint16_t decode[256], uint16_t thresholds[256])
{
    return guard([&] {
        REQUIRE(decode && thresholds, "null argument");
        REQUIRE(transfer == MARAY_TRANSFER_NONE || transfer == MARAY_TRANSFER_SRGB, "unknown transfer");
        static const uint16_t srgb[256] = {MARAY_SRGB_DECODE_LIST};
        for (uint32_t v = 0; v < 256; v++) {
            decode[v] = transfer == MARAY_TRANSFER_SRGB ? srgb[v] : (uint16_t)v;
            thresholds[v] = !v ? 0 : transfer == MARAY_TRANSFER_SRGB ? (uint16_t)(((uint32_t)srgb[v - 1] + srgb[v] + 1) >> 1) : (uint16_t)v;
        }
    });
}

// ---- device PNG encoder (include/maray_hip.h) ----------------------------------------------------------------
static void png_hand_over(const std::vector<uint8_t> &file, uint8_t **png_out, size_t *n_out)
{
    uint8_t *p = (uint8_t *)malloc(file.size() ? file.size() : 1);
    if (!p) throw Error{MARAY_E_INTERNAL, "out of memory"};
    memcpy(p, file.data(), file.size());
    *png_out = p; *n_out = file.size();
}

int maray_hip_png_encode_device(int device, const void *d_rgb8, uint32_t w, uint32_t h, void *stream, uint8_t **png_out, size_t *n_out)
{
    return maray_hip_png_encode_device_ex(device, d_rgb8, w, h, MARAY_PNG_CODES_FIXED, stream, png_out, n_out);
}

// the words of a maray_png_opts (null: all zeros), checked before a device is looked for
static void png_opts_words(const maray_png_opts *opts, uint32_t *codes, uint32_t *filter)
{
    *codes = opts ? opts->codes : (uint32_t)MARAY_PNG_CODES_FIXED;
    *filter = opts ? opts->filter : (uint32_t)MARAY_PNG_FILTER_NONE;
    REQUIRE(*codes == MARAY_PNG_CODES_FIXED || *codes == MARAY_PNG_CODES_DYNAMIC, "unknown PNG codes");
    REQUIRE(png_filter_known(*filter), "unknown PNG filter");
    for (int i = 0; opts && i < 6; i++) REQUIRE(!opts->reserved[i], "maray_png_opts: a reserved word is not 0");
}

int maray_hip_png_encode_device_ex(int device, const void *d_rgb8, uint32_t w, uint32_t h, uint32_t codes, void *stream, uint8_t **png_out,
                                   size_t *n_out)
{
    maray_png_opts o;
    memset(&o, 0, sizeof o);
    o.codes = codes;
    return maray_hip_png_encode_device_opts(device, d_rgb8, w, h, &o, stream, png_out, n_out);
}

int maray_hip_png_encode_device_opts(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_opts *opts, void *stream,
                                     uint8_t **png_out, size_t *n_out)
{
    return guard([&] {
        REQUIRE(png_out && n_out, "null argument");
        *png_out = nullptr; *n_out = 0;
        uint32_t codes, filter;
        png_opts_words(opts, &codes, &filter);
        REQUIRE(d_rgb8, "null argument");
        REQUIRE(w && h, "empty image");
        png_check_size(w, h);
        PngEncoderLease E(device);
        PngPiece piece;
        piece.y0 = 0; piece.y1 = h;
        E->encode_rows((const unsigned char *)d_rgb8, w, h, (hipStream_t)stream, piece, codes, filter);
        png_hand_over(png_assemble(w, h, {&piece}), png_out, n_out);
    });
}

int maray_hip_render_png(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, uint8_t **png_out, size_t *n_out)
{
    return maray_hip_render_png_ex(c, w, h, values, n_frames, MARAY_PNG_CODES_FIXED, png_out, n_out);
}

int maray_hip_render_png_ex(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, uint32_t codes, uint8_t **png_out,
                            size_t *n_out)
{
    maray_png_opts o;
    memset(&o, 0, sizeof o);
    o.codes = codes;
    return maray_hip_render_png_opts(c, w, h, values, n_frames, &o, png_out, n_out);
}

int maray_hip_render_png_opts(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, const maray_png_opts *opts,
                              uint8_t **png_out, size_t *n_out)
{
    return guard([&] {
        REQUIRE(png_out && n_out, "null argument");
        *png_out = nullptr; *n_out = 0;
        uint32_t codes, filter;
        png_opts_words(opts, &codes, &filter);
        REQUIRE(c && c->backend, "null context");
        REQUIRE(w && h, "empty image");
        check_rows(w, h, 0, h);
        png_check_size(w, h);
        check_samples(c, w, h, false, values != nullptr);
        if (values) check_shutter(c, values, n_frames);
        int device = 0;
        {
            std::lock_guard<std::mutex> lk(g_ctx_device_mutex);
            auto it = g_ctx_device.find(c);
            if (it == g_ctx_device.end()) throw Error{MARAY_E_ARG, "unknown context"};
            device = it->second;
        }
        PngEncoderLease E(device);
        PngPiece piece;
        piece.y0 = 0; piece.y1 = h;
        E->encode_rendered(w, 0, h, E->own_stream, [&](uint32_t b0, uint32_t b1, unsigned char *d8, hipStream_t st) {
            if (values) c->backend->render_device_shutter(w, h, RowBlocks::range(b0, b1), values, n_frames, d8, st);
            else c->backend->render_device(w, h, RowBlocks::range(b0, b1), d8, nullptr, st);
        }, piece, codes, filter);
        png_hand_over(png_assemble(w, h, {&piece}), png_out, n_out);
    });
}

int maray_hip_time_png_encode(int device, const void *d_rgb8, uint32_t w, uint32_t h, int reps, float *ms_avg, uint64_t *stream_bytes)
{
    return maray_hip_time_png_encode_ex(device, d_rgb8, w, h, MARAY_PNG_CODES_FIXED, reps, ms_avg, stream_bytes);
}

int maray_hip_time_png_encode_ex(int device, const void *d_rgb8, uint32_t w, uint32_t h, uint32_t codes, int reps, float *ms_avg,
                                 uint64_t *stream_bytes)
{
    maray_png_opts o;
    memset(&o, 0, sizeof o);
    o.codes = codes;
    return maray_hip_time_png_encode_opts(device, d_rgb8, w, h, &o, reps, ms_avg, stream_bytes);
}

int maray_hip_time_png_encode_opts(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_opts *opts, int reps, float *ms_avg,
                                   uint64_t *stream_bytes)
{
    return guard([&] {
        REQUIRE(ms_avg, "null argument");
        uint32_t codes, filter;
        png_opts_words(opts, &codes, &filter);
        *ms_avg = png_time_kernels(device, (const unsigned char *)d_rgb8, w, h, reps, stream_bytes, codes, filter);
    });
}

uint64_t maray_hip_png_bytes_to_host(void) { return png_bytes_to_host(); }

// ---- indexed colour (include/maray_hip.h, "Indexed colour") ---------------------------------------------------------
// the mode of a maray_png_color_opts (null: all zeros), checked before a device is looked for
static uint32_t png_color_mode(const maray_png_color_opts *opts)
{
    const uint32_t color = opts ? opts->color : (uint32_t)MARAY_PNG_COLOR_RGB;
    REQUIRE(color <= MARAY_PNG_COLOR_AUTO, "unknown PNG color mode");
    for (int i = 0; opts && i < 7; i++) REQUIRE(!opts->reserved[i], "maray_png_color_opts: a reserved word is not 0");
    return color;
}

// the decision: true = the indexed file; false = the truecolour file (AUTO); INDEXED on more than 256 colours throws
static bool png_indexed_file(uint32_t color, uint32_t n_colors)
{
    if (n_colors <= 256) return true;
    if (color == MARAY_PNG_COLOR_INDEXED) throw Error{MARAY_E_LIMIT, "the raster holds more than 256 colours"};
    return false;
}

int maray_hip_png_encode_device_color(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_color_opts *opts, void *stream,
                                      uint8_t **png_out, size_t *n_out)
{
    uint32_t color = MARAY_PNG_COLOR_RGB;
    const int rc = guard([&] {
        REQUIRE(png_out && n_out, "null argument");
        *png_out = nullptr; *n_out = 0;
        color = png_color_mode(opts);
        if (color == MARAY_PNG_COLOR_RGB) return;
        REQUIRE(d_rgb8, "null argument");
        REQUIRE(w && h, "empty image");
        png_check_size(w, h);
        PngEncoderLease E(device);
        const unsigned char *src = (const unsigned char *)d_rgb8;
        const hipStream_t st = (hipStream_t)stream;
        uint8_t palette[768];
        E->collect_colors(src, (uint64_t)w * h, st, false);
        const uint32_t n = E->fetch_palette(st, palette);
        PngPiece piece;
        piece.y0 = 0; piece.y1 = h;
        if (png_indexed_file(color, n)) {
            E->encode_rows_indexed(src, w, h, n, st, piece);
            png_hand_over(png_assemble_indexed(w, h, palette, n, {&piece}), png_out, n_out);
        } else {
            E->encode_rows(src, w, h, st, piece);
            png_hand_over(png_assemble(w, h, {&piece}), png_out, n_out);
        }
    });
    if (rc == MARAY_OK && color == MARAY_PNG_COLOR_RGB) return maray_hip_png_encode_device(device, d_rgb8, w, h, stream, png_out, n_out);
    return rc;
}

int maray_hip_render_png_color(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_frames, const maray_png_color_opts *opts,
                               uint8_t **png_out, size_t *n_out)
{
    uint32_t color = MARAY_PNG_COLOR_RGB;
    const int rc = guard([&] {
        REQUIRE(png_out && n_out, "null argument");
        *png_out = nullptr; *n_out = 0;
        color = png_color_mode(opts);
        if (color == MARAY_PNG_COLOR_RGB) return;
        REQUIRE(c && c->backend, "null context");
        REQUIRE(w && h, "empty image");
        check_rows(w, h, 0, h);
        png_check_size(w, h);
        check_samples(c, w, h, false, values != nullptr);
        if (values) check_shutter(c, values, n_frames);
        int device = 0;
        {
            std::lock_guard<std::mutex> lk(g_ctx_device_mutex);
            auto it = g_ctx_device.find(c);
            if (it == g_ctx_device.end()) throw Error{MARAY_E_ARG, "unknown context"};
            device = it->second;
        }
        PngEncoderLease E(device);
        const hipStream_t st = E->own_stream;
        auto render = [&](uint32_t b0, uint32_t b1, unsigned char *d8, hipStream_t s) {
            if (values) c->backend->render_device_shutter(w, h, RowBlocks::range(b0, b1), values, n_frames, d8, s);
            else c->backend->render_device(w, h, RowBlocks::range(b0, b1), d8, nullptr, s);
        };
        const uint32_t step = E->band_rows(w);
        unsigned char *d8 = E->band_buffer((size_t)std::min(step, h) * w * 3);
        // the colours: band by band into one palette; an image of one band stays in the band buffer
        for (uint32_t b0 = 0; b0 < h; b0 += step) {
            const uint32_t b1 = b0 + std::min(step, h - b0);
            render(b0, b1, d8, st);
            E->collect_colors(d8, (uint64_t)(b1 - b0) * w, st, b0 != 0);
        }
        uint8_t palette[768];
        const uint32_t n = E->fetch_palette(st, palette);
        PngPiece piece;
        piece.y0 = 0; piece.y1 = h;
        if (!png_indexed_file(color, n)) {
            if (h <= step) E->encode_rows(d8, w, h, st, piece);
            else E->encode_rendered(w, 0, h, st, render, piece);
            png_hand_over(png_assemble(w, h, {&piece}), png_out, n_out);
            return;
        }
        for (uint32_t b0 = 0; b0 < h; b0 += step) {
            const uint32_t b1 = b0 + std::min(step, h - b0);
            if (h > step) render(b0, b1, d8, st);               // (the second render of a band)
            E->encode_rows_indexed(d8, w, b1 - b0, n, st, piece);
        }
        png_hand_over(png_assemble_indexed(w, h, palette, n, {&piece}), png_out, n_out);
    });
    if (rc == MARAY_OK && color == MARAY_PNG_COLOR_RGB) return maray_hip_render_png(c, w, h, values, n_frames, png_out, n_out);
    return rc;
}

int maray_hip_time_png_encode_color(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_png_color_opts *opts, int reps, float *ms_avg,
                                    uint64_t *stream_bytes)
{
    uint32_t color = MARAY_PNG_COLOR_RGB;
    const int rc = guard([&] {
        REQUIRE(ms_avg, "null argument");
        color = png_color_mode(opts);
        if (color != MARAY_PNG_COLOR_RGB) *ms_avg = png_time_kernels_color(device, (const unsigned char *)d_rgb8, w, h, color, reps, stream_bytes);
    });
    if (rc == MARAY_OK && color == MARAY_PNG_COLOR_RGB) return maray_hip_time_png_encode(device, d_rgb8, w, h, reps, ms_avg, stream_bytes);
    return rc;
}

int maray_hip_png_palette(int device, const void *d_rgb8, uint32_t w, uint32_t h, void *stream, uint32_t *n_colors, uint8_t palette[768])
{
    return guard([&] {
        REQUIRE(n_colors && palette && d_rgb8, "null argument");
        *n_colors = 0;
        REQUIRE(w && h, "empty image");
        png_check_size(w, h);
        PngEncoderLease E(device);
        E->collect_colors((const unsigned char *)d_rgb8, (uint64_t)w * h, (hipStream_t)stream, false);
        *n_colors = E->fetch_palette((hipStream_t)stream, palette);
    });
}

// ---- animation (include/maray_hip.h) ---------------------------------------------------------------------------
int maray_hip_frame_delta(int device, const void *d_prev, const void *d_cur, uint32_t w, uint32_t h, void *stream, uint32_t box[4])
{
    return guard([&] {
        REQUIRE(d_prev && d_cur && box, "null argument");
        REQUIRE(w && h, "empty image");
        apng_check_frame(w, h);
        frame_delta_once(device, (const unsigned char *)d_prev, (const unsigned char *)d_cur, w, h, (hipStream_t)stream, box);
    });
}

int maray_hip_apng_encode_device(int device, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, uint32_t delay_num,
                                 uint32_t delay_den, uint32_t n_plays, void *stream, uint8_t **out, size_t *n_out)
{
    return guard([&] {
        REQUIRE(out && n_out, "null argument");
        *out = nullptr; *n_out = 0;
        REQUIRE(d_frames, "null argument");
        apng_check_timing(n_frames, delay_num, delay_den);
        REQUIRE(w && h, "empty image");
        apng_check_frame(w, h);
        PngEncoderLease E(device);
        ApngWriter W(*E.e, w, h, n_frames, delay_num, delay_den, n_plays);
        const size_t pitch = (size_t)w * 3;
        for (uint32_t i = 0; i < n_frames; i++) {
            const unsigned char *frame = (const unsigned char *)d_frames + (size_t)i * pitch * h;
            W.add_frame([&](uint32_t b0, uint32_t b1, unsigned char *d8, hipStream_t st) {
                const hipError_t e = hipMemcpyAsync(d8, frame + (size_t)b0 * pitch, (size_t)(b1 - b0) * pitch, hipMemcpyDeviceToDevice, st);
                if (e != hipSuccess) throw Error{MARAY_E_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e)};
            }, (hipStream_t)stream);
        }
        png_hand_over(W.finish(), out, n_out);
    });
}

int maray_hip_render_apng(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub,
                          uint32_t delay_num, uint32_t delay_den, uint32_t n_plays, uint8_t **out, size_t *n_out)
{
    return maray::render_apng_codes(c, w, h, values, n_images, n_sub, delay_num, delay_den, n_plays, MARAY_PNG_CODES_FIXED, out, n_out);
}

// maray_hip_render_apng with the frames' codes (apng_device.hpp): maray_gen_animation's way in
extern "C++" int maray::render_apng_codes(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub,
                             uint32_t delay_num, uint32_t delay_den, uint32_t n_plays, uint32_t codes, uint8_t **out, size_t *n_out)
{
    return guard([&] {
        REQUIRE(codes == MARAY_PNG_CODES_FIXED || codes == MARAY_PNG_CODES_DYNAMIC, "unknown PNG codes");
        REQUIRE(out && n_out, "null argument");
        *out = nullptr; *n_out = 0;
        REQUIRE(c && c->backend, "null context");
        apng_check_timing(n_images, delay_num, delay_den);
        REQUIRE(w && h, "empty image");
        check_rows(w, h, 0, h);
        apng_check_frame(w, h);
        check_samples(c, w, h, false, true);
        // every row of every image, before the first launch
        const size_t P = c->param_ranges.size() / 2;
        for (uint32_t i = 0; i < n_images; i++) check_shutter(c, values ? values + (size_t)i * n_sub * P : nullptr, n_sub);
        int device = 0;
        {
            std::lock_guard<std::mutex> lk(g_ctx_device_mutex);
            auto it = g_ctx_device.find(c);
            if (it == g_ctx_device.end()) throw Error{MARAY_E_ARG, "unknown context"};
            device = it->second;
        }
        PngEncoderLease E(device);
        ApngWriter W(*E.e, w, h, n_images, delay_num, delay_den, n_plays, codes);
        for (uint32_t i = 0; i < n_images; i++) {
            const double *rows = values ? values + (size_t)i * n_sub * P : nullptr;
            W.add_frame([&](uint32_t b0, uint32_t b1, unsigned char *d8, hipStream_t st) {
                c->backend->render_device_shutter(w, h, RowBlocks::range(b0, b1), rows, n_sub, d8, st);
            }, E->own_stream);
        }
        png_hand_over(W.finish(), out, n_out);
    });
}

int maray_hip_time_frame_delta_copy(int device, uint32_t w, uint32_t h, int reps, float *ms_avg, float *copy_ms_avg)
{
    return guard([&] {
        REQUIRE(ms_avg, "null argument");
        *ms_avg = frame_delta_time(device, w, h, reps, copy_ms_avg);
    });
}

int maray_hip_time_frame_delta(int device, uint32_t w, uint32_t h, int reps, float *ms_avg)
{
    return maray_hip_time_frame_delta_copy(device, w, h, reps, ms_avg, nullptr);
}

// ---- raw video (include/maray_hip.h) ----------------------------------------------------------------------------
int maray_ycc_frame_bytes(uint32_t w, uint32_t h, uint32_t sampling, size_t *out)
{
    return guard([&] {
        REQUIRE(out, "null argument");
        *out = 0;
        REQUIRE(sampling == MARAY_YCC_420 || sampling == MARAY_YCC_444, "unknown Y'CbCr sampling");
        *out = ycc_frame_bytes(w, h, sampling);
    });
}

int maray_hip_rgb_to_ycc(int device, const void *d_rgb8, uint32_t w, uint32_t h, const maray_ycc_opts *opts, void *d_planes, void *stream)
{
    return guard([&] {
        REQUIRE(d_rgb8 && d_planes, "null argument");
        uint32_t sampling, matrix;
        ycc_opts_words(opts, &sampling, &matrix);
        ycc_check_frame(w, h);
        const hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) throw Error{MARAY_E_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e)};
        rgb_to_ycc((const unsigned char *)d_rgb8, w, h, sampling, matrix, (unsigned char *)d_planes, (hipStream_t)stream);
    });
}

// The file of the entry points that return it: malloc'ed once for the whole file where its size is known in front, written by
// the sink straight from the pinned planes, and handed to the caller as it is (maray_free) -- no second copy of the video.
extern "C++" {
struct Y4mFile {
    uint8_t *p = nullptr; size_t cap = 0, n = 0;
    ~Y4mFile() { free(p); }
    void reserve(size_t want) {
        if (want <= cap) return;
        uint8_t *q = (uint8_t *)realloc(p, want);
        if (!q) throw Error{MARAY_E_INTERNAL, "out of memory"};
        p = q; cap = want;
    }
    void put(const void *src, size_t bytes) {
        if (n + bytes > cap) reserve(std::max(n + bytes, cap + cap / 2));
        memcpy(p + n, src, bytes);
        n += bytes;
    }
    void hand_over(uint8_t **out, size_t *n_out) { reserve(1); *out = p; *n_out = n; p = nullptr; cap = n = 0; }
    Y4mWriter::Sink sink() { return [this](const void *src, size_t bytes) { put(src, bytes); }; }
};
}

int maray_hip_y4m_encode_device(int device, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t h, uint32_t delay_num,
                                uint32_t delay_den, const maray_ycc_opts *opts, void *stream, uint8_t **out, size_t *n_out)
{
    return guard([&] {
        REQUIRE(out && n_out, "null argument");
        *out = nullptr; *n_out = 0;
        REQUIRE(d_frames, "null argument");
        uint32_t sampling, matrix;
        ycc_opts_words(opts, &sampling, &matrix);
        y4m_check_timing(n_frames, delay_num, delay_den);
        ycc_check_frame(w, h);
        Y4mFile file;
        Y4mWriter W(device, w, h, n_frames, delay_num, delay_den, sampling, matrix, file.sink());
        file.reserve(W.header.size() + (size_t)n_frames * (6 + W.frame_bytes));
        for (uint32_t i = 0; i < n_frames; i++) W.add_frame((const unsigned char *)d_frames + (size_t)i * w * 3 * h, (hipStream_t)stream);
        W.finish();
        file.hand_over(out, n_out);
    });
}

int maray_hip_render_y4m(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub,
                         uint32_t delay_num, uint32_t delay_den, const maray_ycc_opts *opts, uint8_t **out, size_t *n_out)
{
    if (!out || !n_out) return fail(MARAY_E_ARG, "null argument");
    *out = nullptr; *n_out = 0;
    Y4mFile file;
    // (room for the whole file at once where the arguments are in range -- a header line is under 128 bytes; render_y4m_to
    // checks them)
    if (n_images && w && h && (uint64_t)w * 3 * h <= YCC_FRAME_MAX_BYTES && (!opts || opts->sampling <= MARAY_YCC_444)) {
        const int rc = guard([&] { file.reserve(128 + (size_t)n_images * (6 + ycc_frame_bytes(w, h, opts ? opts->sampling : (uint32_t)MARAY_YCC_420))); });
        if (rc) return rc;
    }
    if (const int rc = maray::render_y4m_to(c, w, h, values, n_images, n_sub, delay_num, delay_den, opts, file.sink())) return rc;
    return guard([&] { file.hand_over(out, n_out); });
}

// maray_hip_render_y4m into a sink (y4m_device.hpp): maray_gen_animation_ex's way in
extern "C++" int maray::render_y4m_to(maray_ctx *c, uint32_t w, uint32_t h, const double *values, uint32_t n_images, uint32_t n_sub,
                                     uint32_t delay_num, uint32_t delay_den, const maray_ycc_opts *opts, const Y4mWriter::Sink &sink)
{
    return guard([&] {
        uint32_t sampling, matrix;
        ycc_opts_words(opts, &sampling, &matrix);
        y4m_check_timing(n_images, delay_num, delay_den);
        ycc_check_frame(w, h);
        REQUIRE(c && c->backend, "null context");
        check_rows(w, h, 0, h);
        check_samples(c, w, h, false, true);
        // every row of every image, before the first launch
        const size_t P = c->param_ranges.size() / 2;
        for (uint32_t i = 0; i < n_images; i++) check_shutter(c, values ? values + (size_t)i * n_sub * P : nullptr, n_sub);
        int device = 0;
        {
            std::lock_guard<std::mutex> lk(g_ctx_device_mutex);
            auto it = g_ctx_device.find(c);
            if (it == g_ctx_device.end()) throw Error{MARAY_E_ARG, "unknown context"};
            device = it->second;
        }
        Y4mWriter W(device, w, h, n_images, delay_num, delay_den, sampling, matrix, sink);
        // (the device's render stream, not one of this call's: the back-end keeps the stream of its last launch)
        const hipStream_t st = y4m_render_stream(device);
        struct Drain {
            hipStream_t st;
            ~Drain() { (void)hipStreamSynchronize(st); }
        } drain{st};    // (declared after W: the renders are waited for before the writer's buffers go)
        for (uint32_t i = 0; i < n_images; i++) {
            c->backend->render_device_shutter(w, h, RowBlocks::range(0, h), values ? values + (size_t)i * n_sub * P : nullptr, n_sub, W.raster(), st);
            W.add_frame(W.raster(), st);
        }
        W.finish();
    });
}

int maray_hip_time_rgb_to_ycc(int device, uint32_t w, uint32_t h, const maray_ycc_opts *opts, int reps, float *ms_avg, float *copy_ms_avg)
{
    return guard([&] {
        REQUIRE(ms_avg, "null argument");
        uint32_t sampling, matrix;
        ycc_opts_words(opts, &sampling, &matrix);
        *ms_avg = rgb_to_ycc_time(device, w, h, sampling, matrix, reps, copy_ms_avg);
    });
}

int maray_host_alloc(size_t bytes, void **out)
{
    return guard([&] {
        REQUIRE(out, "null argument");
        *out = host_alloc_pinned(bytes);
    });
}

void maray_host_free(void *p) { host_free_pinned(p); }

int maray_host_register(void *p, size_t bytes)
{
    return guard([&] { REQUIRE(p && bytes, "null argument"); host_register(p, bytes); });
}

int maray_host_unregister(void *p)
{
    return guard([&] { REQUIRE(p, "null argument"); host_unregister(p); });
}

int maray_hip_render_rows_device(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1,
                                 void *d_rgb8, void *d_rgb64, void *stream)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        check_rows(w, h, y0, y1);
        check_samples(c, w, h, d_rgb64 != nullptr);
        if (y0 == y1 || w == 0) return;
        c->backend->render_device(w, h, RowBlocks::range(y0, y1), d_rgb8, d_rgb64, stream);
    });
}

int maray_hip_render_blocks_device(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t block_rows, uint32_t block_stride,
                                   uint32_t n_blocks, void *d_rgb8, void *d_rgb64, void *stream)
{
    return guard([&] {
        REQUIRE(c && c->backend, "null context");
        if (n_blocks == 0 || block_rows == 0 || w == 0) return;
        REQUIRE(n_blocks == 1 || block_stride >= block_rows, "row blocks overlap: block_stride < block_rows");
        const uint64_t last = (uint64_t)y0 + (uint64_t)(n_blocks - 1) * block_stride + block_rows;       // one past the last row
        REQUIRE(last <= 0xFFFFFFFFull && (uint64_t)n_blocks * block_rows <= 0xFFFFFFFFull, "row blocks out of range");
        check_rows(w, h, y0, (uint32_t)last);
        check_samples(c, w, h, d_rgb64 != nullptr);
        c->backend->render_device(w, h, RowBlocks{y0, n_blocks * block_rows, block_rows, n_blocks == 1 ? 0u : block_stride}, d_rgb8, d_rgb64, stream);
    });
}

int maray_hip_time_rows(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t y1,
                        void *d_rgb8, void *d_rgb64, int reps, float *ms_avg)
{
    return guard([&] {
        REQUIRE(c && c->backend && ms_avg, "null argument");
        check_rows(w, h, y0, y1);
        check_samples(c, w, h, d_rgb64 != nullptr);
        REQUIRE(y1 > y0 && w > 0 && reps > 0, "empty launch");
        *ms_avg = c->backend->time_rows(w, h, RowBlocks::range(y0, y1), d_rgb8, d_rgb64, reps);
    });
}

int maray_hip_time_blocks(maray_ctx *c, uint32_t w, uint32_t h, uint32_t y0, uint32_t block_rows, uint32_t block_stride,
                          uint32_t n_blocks, void *d_rgb8, void *d_rgb64, int reps, float *ms_avg)
{
    return guard([&] {
        REQUIRE(c && c->backend && ms_avg, "null argument");
        REQUIRE(n_blocks > 0 && block_rows > 0 && w > 0 && reps > 0, "empty launch");
        REQUIRE(n_blocks == 1 || block_stride >= block_rows, "row blocks overlap: block_stride < block_rows");
        const uint64_t last = (uint64_t)y0 + (uint64_t)(n_blocks - 1) * block_stride + block_rows;
        REQUIRE(last <= 0xFFFFFFFFull && (uint64_t)n_blocks * block_rows <= 0xFFFFFFFFull, "row blocks out of range");
        check_rows(w, h, y0, (uint32_t)last);
        check_samples(c, w, h, d_rgb64 != nullptr);
        *ms_avg = c->backend->time_rows(w, h, RowBlocks{y0, n_blocks * block_rows, block_rows, n_blocks == 1 ? 0u : block_stride}, d_rgb8, d_rgb64, reps);
    });
}

int maray_jit_source(const maray_program *prog, char **src_out)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        const std::string s = jit_source(*prog);
        *src_out = (char *)malloc(s.size() + 1);
        if (!*src_out) throw Error{MARAY_E_INTERNAL, "out of memory"};
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_jit_source_samples(const maray_program *prog, uint32_t k, char **src_out)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        const std::string s = jit_source_samples(*prog, k);
        *src_out = (char *)malloc(s.size() + 1);
        if (!*src_out) throw Error{MARAY_E_INTERNAL, "out of memory"};
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_jit_source_rows(const maray_program *prog, char **src_out, uint32_t *n_chunks)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        const std::string s = jit_source_rows(*prog, n_chunks);
        *src_out = (char *)malloc(s.size() + 1);
        if (!*src_out) throw Error{MARAY_E_INTERNAL, "out of memory"};
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_row_cone(const maray_program *prog, uint32_t first_out, uint32_t n_out, uint64_t **ops_out, uint32_t *n_ops_out, uint32_t *n_slots_out)
{
    return guard([&] {
        REQUIRE(prog && ops_out && n_ops_out && n_slots_out, "null argument");
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        validate_program(*prog);
        const RowTapeDeps deps = row_tape_deps(*prog);
        std::vector<uint32_t> outs;
        for (uint32_t o : deps.outs) {
            const uint32_t k = MARAY_INS_AUX(prog->row_ops[o]);
            if (k >= first_out && k - first_out < n_out) outs.push_back(o);
        }
        std::vector<uint64_t> t = compact_tape(row_tape_cone(*prog, deps, outs, nullptr));
        *n_slots_out = getenv("MARAY_TAPE_KEEP_ORDER") ? renumber_slots(t) : reschedule_tape(t);
        *n_ops_out = (uint32_t)t.size();
        *ops_out = (uint64_t *)malloc(t.size() * 8 + 8);
        if (!*ops_out) throw Error{MARAY_E_INTERNAL, "out of memory"};
        memcpy(*ops_out, t.data(), t.size() * 8);
    });
}

int maray_jit_build(const maray_program *prog, void **code_out, size_t *len_out)
{
    return guard([&] {
        REQUIRE(prog && code_out && len_out, "null argument");
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        // both kernels, through the code object cache (this is also how a cache is warmed ahead of a render)
        const std::vector<char> &code = jit_code_for(*prog)->pix;
        *code_out = malloc(code.size() ? code.size() : 1);
        if (!*code_out) throw Error{MARAY_E_INTERNAL, "out of memory"};
        memcpy(*code_out, code.data(), code.size());
        *len_out = code.size();
    });
}

int maray_jit_build_samples(const maray_program *prog, uint32_t k, void **code_out, size_t *len_out)
{
    return guard([&] {
        REQUIRE(prog && code_out && len_out, "null argument");
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        const std::shared_ptr<const std::vector<char>> code = jit_code_samples(*prog, k);
        *code_out = malloc(code->size() ? code->size() : 1);
        if (!*code_out) throw Error{MARAY_E_INTERNAL, "out of memory"};
        memcpy(*code_out, code->data(), code->size());
        *len_out = code->size();
    });
}

int maray_jit_code_key(const maray_program *prog, char *out33)
{
    return guard([&] {
        REQUIRE(prog && out33, "null argument");
        const maray_program loaded = load_program(prog);
        prog = &loaded;
        const std::string k = jit_code_key(*prog);
        memcpy(out33, k.c_str(), std::min<size_t>(k.size(), 32) + 1);
        out33[32] = 0;
    });
}

int maray_jit_code_cached(const maray_program *prog, int *cached)
{
    return guard([&] { REQUIRE(prog && cached, "null argument"); *cached = jit_code_is_cached(load_program(prog)) ? 1 : 0; });
}

int maray_jit_source_refine(const maray_program *prog, const maray_refine *refine, char **src_out)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        std::string s;
        if (refine && refine->n_ops) { validate_refine(loaded, *refine); s = jit_source_refine(loaded, *refine); }
        *src_out = (char *)malloc(s.size() + 1);
        REQUIRE(*src_out, "out of memory");
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_jit_build_refine(const maray_program *prog, const maray_refine *refine, void **code_out, size_t *len_out)
{
    return guard([&] {
        REQUIRE(prog && refine && code_out && len_out, "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        *code_out = nullptr; *len_out = 0;
        if (!refine->n_ops) return;
        validate_refine(loaded, *refine);
        const std::shared_ptr<const JitRefineCode> c = jit_code_refine(loaded, *refine);
        if (!c) return;
        *code_out = malloc(c->code.size());
        REQUIRE(*code_out, "out of memory");
        memcpy(*code_out, c->code.data(), c->code.size());
        *len_out = c->code.size();
    });
}

int maray_jit_guard_layout(const maray_program *prog, int32_t *pos, uint32_t cap, uint32_t *n_guards, uint32_t *n_words, uint32_t *gw, uint32_t *gh)
{
    return guard([&] {
        REQUIRE(prog && n_guards && n_words && gw && gh && (pos || !cap), "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        std::vector<int32_t> p;
        jit_guard_layout(loaded, p, n_words, gw, gh);
        *n_guards = (uint32_t)p.size();
        for (uint32_t g = 0; g < p.size() && g < cap; g++) pos[g] = p[g];
    });
}

int maray_hip_refine_count(const maray_ctx *c, uint64_t *refine_passes)
{
    return guard([&] { REQUIRE(c && c->backend && refine_passes, "null argument"); *refine_passes = c->backend->refine_count(); });
}

int maray_hip_census_count(const maray_ctx *c, uint64_t *census_launches)
{
    return guard([&] { REQUIRE(c && c->backend && census_launches, "null argument"); *census_launches = c->backend->census_count(); });
}

int maray_jit_census_eligible(const maray_program *prog, uint64_t *mask, uint32_t cap, uint32_t *n_words)
{
    return guard([&] {
        REQUIRE(prog && n_words && (mask || !cap), "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        std::vector<uint64_t> el;
        (void)jit_source_census(loaded, &el);
        std::vector<int32_t> pos;
        uint32_t nw = 0, gw = 0, gh = 0;
        jit_guard_layout(loaded, pos, &nw, &gw, &gh);
        el.resize(nw, 0);                               // no kernel: no bit is eligible
        *n_words = (uint32_t)el.size();
        for (uint32_t j = 0; j < el.size() && j < cap; j++) mask[j] = el[j];
    });
}

int maray_jit_source_census(const maray_program *prog, char **src_out)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        const std::string s = jit_source_census(loaded);
        *src_out = (char *)malloc(s.size() + 1);
        REQUIRE(*src_out, "out of memory");
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_hip_debug_guard_words(maray_ctx *c, uint64_t *words, size_t cap, size_t *n_words, uint32_t *words_per_rect)
{
    return guard([&] {
        REQUIRE(c && c->backend && n_words && words_per_rect && (words || !cap), "null argument");
        *n_words = c->backend->debug_guard_words(words, cap, words_per_rect);
    });
}

int maray_hip_debug_census_words(maray_ctx *c, uint64_t *words, size_t cap, size_t *n_words, uint32_t *words_per_rect)
{
    return guard([&] {
        REQUIRE(c && c->backend && n_words && words_per_rect && (words || !cap), "null argument");
        *n_words = c->backend->debug_census_words(words, cap, words_per_rect);
    });
}

int maray_hip_cover_count(const maray_ctx *c, uint64_t *cover_launches)
{
    return guard([&] { REQUIRE(c && c->backend && cover_launches, "null argument"); *cover_launches = c->backend->cover_count(); });
}

int maray_jit_cover_bits(const maray_program *prog, int32_t *values, uint32_t cap, uint32_t *n_values)
{
    return guard([&] {
        REQUIRE(prog && n_values && (values || !cap), "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        const CoverPlan cp = jit_cover_plan(loaded);
        std::vector<int32_t> v{(int32_t)cp.reds.size()};
        for (const CoverPlan::Red &r : cp.reds) {
            v.insert(v.end(), {r.bit, (int32_t)r.root, (int32_t)r.leaf_end.size()});
            for (size_t k = 0; k < r.leaf_end.size(); k++) v.insert(v.end(), {(int32_t)r.leaf_end[k], (int32_t)r.leaf_bit[k], (int32_t)r.leaf_taint[k], (int32_t)r.leaf_eligible[k]});
        }
        *n_values = (uint32_t)v.size();
        for (uint32_t j = 0; j < v.size() && j < cap; j++) values[j] = v[j];
    });
}

int maray_jit_source_cover(const maray_program *prog, char **src_out)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        const std::string s = jit_source_cover(loaded);
        *src_out = (char *)malloc(s.size() + 1);
        REQUIRE(*src_out, "out of memory");
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_hip_debug_cover_words(maray_ctx *c, uint64_t *words, size_t cap, size_t *n_words, uint32_t *words_per_rect)
{
    return guard([&] {
        REQUIRE(c && c->backend && n_words && words_per_rect && (words || !cap), "null argument");
        *n_words = c->backend->debug_cover_words(words, cap, words_per_rect);
    });
}

int maray_hip_rowscan_count(const maray_ctx *c, uint64_t *rowscan_launches)
{
    return guard([&] { REQUIRE(c && c->backend && rowscan_launches, "null argument"); *rowscan_launches = c->backend->rowscan_count(); });
}

int maray_jit_rowwords_flag(const maray_program *prog, int32_t *flag_bit)
{
    return guard([&] {
        REQUIRE(prog && flag_bit, "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        *flag_bit = jit_rowwords_plan(loaded).flag_bit;
    });
}

int maray_jit_source_rowwords(const maray_program *prog, char **src_out)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        const std::string s = jit_source_rowwords(loaded);
        *src_out = (char *)malloc(s.size() + 1);
        REQUIRE(*src_out, "out of memory");
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_hip_prepass_count(const maray_ctx *c, uint64_t *prepass_launches)
{
    return guard([&] { REQUIRE(c && c->backend && prepass_launches, "null argument"); *prepass_launches = c->backend->prepass_count(); });
}

int maray_hip_deferred_count(maray_ctx *c, uint64_t *deferred_tiles)
{
    return guard([&] { REQUIRE(c && c->backend && deferred_tiles, "null argument"); *deferred_tiles = c->backend->deferred_count(); });
}

int maray_jit_source_prepass(const maray_program *prog, char **src_out)
{
    return guard([&] {
        REQUIRE(prog && src_out, "null argument");
        const maray_program loaded = load_program(prog);
        validate_program(loaded);
        const std::string s = jit_source_prepass(loaded);
        *src_out = (char *)malloc(s.size() + 1);
        REQUIRE(*src_out, "out of memory");
        memcpy(*src_out, s.c_str(), s.size() + 1);
    });
}

int maray_hip_debug_row_words(maray_ctx *c, uint64_t *xbits, size_t xcap, size_t *n_xbits, uint64_t *rwords, size_t rcap, size_t *n_rwords,
                              uint32_t *words_per_rect, int *used)
{
    return guard([&] {
        REQUIRE(c && c->backend && n_xbits && n_rwords && words_per_rect && used && (xbits || !xcap) && (rwords || !rcap), "null argument");
        *n_xbits = c->backend->debug_row_words(xbits, xcap, rwords, rcap, n_rwords, words_per_rect, used);
    });
}

int maray_hip_debug_row_sets(const maray_ctx *c, int32_t *set, uint32_t *kept_sets, uint64_t *kept_bytes, uint64_t *budget_bytes, uint64_t *held_bytes)
{
    return guard([&] {
        REQUIRE(c && c->backend && set && kept_sets && kept_bytes && budget_bytes && held_bytes, "null argument");
        int s = -1;
        c->backend->debug_row_sets(&s, kept_sets, kept_bytes, budget_bytes, held_bytes);
        *set = s;
    });
}

const char *maray_hip_kernel_name(const maray_ctx *c) { return (c && c->backend) ? c->backend->kernel_name() : ""; }

int maray_hip_launch_counts(const maray_ctx *c, uint64_t *row_passes, uint64_t *order_kernels)
{
    return guard([&] { REQUIRE(c && c->backend && row_passes && order_kernels, "null argument"); c->backend->launch_counts(row_passes, order_kernels); });
}

void maray_free(void *p) { free(p); }

}   // extern "C"
