// png_device.cpp — the object behind the device PNG encoder (product code; include/maray_hip.h, "device PNG encoder"): it
// owns the kernels' scratch (slots, lengths, offsets, the gathered stream), a band buffer for the entry points that render,
// pinned staging and a stream, cuts a raster into bands of rows, and per band brings first the totals (24 bytes) and then
// exactly the compressed bytes to the host.  png_assemble puts the zlib stream and the container around the pieces.
// With MARAY_PNG_CODES_DYNAMIC a band's counts come to the host first, which fits the band's Huffman code
// (maray_png_dynamic_codes' code: lengths, canonical codes, the block header) and closes the band's piece behind the device's bits.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "backend.hpp"
#include "png_container.hpp"
#include "png_device.hpp"

namespace maray {

namespace {

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            throw Error{MARAY_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};           \
    } while (0)

void grow(unsigned char *&p, size_t &cap, size_t want)
{
    if (want <= cap) return;
    if (p) HIP_TRY(hipFree(p));
    p = nullptr; cap = 0;
    HIP_TRY(hipMalloc((void **)&p, want));
    cap = want;
}

std::atomic<uint64_t> g_bytes_to_host{0};

size_t up16(size_t n) { return (n + 15) / 16 * 16; }

uint32_t band_rows_from_env()
{
    const char *e = getenv("MARAY_PNG_BAND_ROWS");
    if (!e || atoll(e) <= 0) return 0;
    return (uint32_t)std::min<long long>(atoll(e), 0x7FFFFFFF);
}

// the scratch of a band of `rows` rows: where everything lies, and the kernels' arguments
PngBandArgs band_args(PngEncoder &E, const unsigned char *src, uint32_t w, uint32_t rows, uint32_t codes = MARAY_PNG_CODES_FIXED,
                      uint32_t filter = MARAY_PNG_FILTER_NONE, const unsigned char *above = nullptr)
{
    const bool dyn = codes == MARAY_PNG_CODES_DYNAMIC;
    PngBandArgs a{};
    a.src = src; a.w = w; a.rows = rows;
    a.nseg = png_row_segments(w);
    a.slot_bytes = dyn ? png_slot_bytes_dyn(w) : png_slot_bytes(w);
    a.codes = codes;
    const uint64_t n = (uint64_t)rows * a.nseg;
    if (n > 0x7FFFFFFFull) throw Error{MARAY_E_INTERNAL, "device PNG encoder: band too large"};
    a.n_segs = (uint32_t)n;
    const size_t payload = (size_t)n * a.slot_bytes;
    grow(E.slots, E.slots_cap, payload);
    grow(E.stream, E.stream_cap, payload + (dyn ? 512 : 0));      // (dynamic: the header's bits and whole dwords at the end)
    const size_t o_adler = up16((size_t)n * 4), o_off = o_adler + up16((size_t)n * 8), o_tot = o_off + up16((size_t)n * 8);
    const size_t o_hist = o_tot + 32, hist_bytes = dyn ? ((size_t)png_hist_blocks(a.n_segs) + 2) * PNG_HIST_STRIDE * 4 : 0;
    grow(E.meta, E.meta_cap, o_hist + hist_bytes);
    if (dyn) a.hist = (uint32_t *)(E.meta + o_hist);            // the blocks' counts, their sums, then the band's code table
    a.slots = E.slots; a.stream = E.stream;
    a.lens = (uint32_t *)E.meta;
    a.adler = (uint32_t *)(E.meta + o_adler);
    a.offsets = (uint64_t *)(E.meta + o_off);
    a.totals = (uint64_t *)(E.meta + o_tot);
    if (filter != MARAY_PNG_FILTER_NONE) {                     // the rows' types, then (ADAPTIVE) ten words per segment
        const size_t o_cost = up16(rows);
        grow(E.filt, E.filt_cap, o_cost + (filter == MARAY_PNG_FILTER_ADAPTIVE ? (size_t)n * 40 : 0));
        a.filter = filter; a.above = above;
        a.row_filter = E.filt;
        if (filter == MARAY_PNG_FILTER_ADAPTIVE) a.cost = (uint32_t *)(E.filt + o_cost);
    }
    return a;
}

}   // namespace

void png_grow(unsigned char *&p, size_t &cap, size_t want) { grow(p, cap, want); }

PngEncoder::PngEncoder(int dev) : device(dev), band_rows_env(band_rows_from_env())
{
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
    HIP_TRY(hipHostMalloc((void **)&h_totals, 32, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void **)&h_counts, (size_t)2 * PNG_HIST_STRIDE * 4, hipHostMallocDefault));
}

PngEncoder::~PngEncoder()
{
    (void)hipSetDevice(device);
    if (own_stream) { (void)hipStreamSynchronize(own_stream); (void)hipStreamDestroy(own_stream); }
    (void)hipFree(slots); (void)hipFree(stream); (void)hipFree(meta); (void)hipFree(raster); (void)hipFree(filt); (void)hipFree(carry);
    (void)hipFree(index); (void)hipFree(colors);
    if (h_palette) (void)hipHostFree(h_palette);
    if (staging) (void)hipHostFree(staging);
    if (h_totals) (void)hipHostFree(h_totals);
    if (h_counts) (void)hipHostFree(h_counts);
}

// Rows of one band: the byte budget (or MARAY_PNG_BAND_ROWS), and never more than 2^30 filtered bytes, so that every size
// and offset inside a band fits 32 bits with room to spare (past a band they are 64-bit)
uint32_t PngEncoder::band_rows(uint32_t w, uint32_t codes) const
{
    const uint64_t row = (uint64_t)w * 3 + 1;
    const uint64_t want = band_rows_env ? band_rows_env : std::max<uint64_t>(1, band_bytes / row);
    const uint64_t most = codes == MARAY_PNG_CODES_DYNAMIC ? PNG_DYN_BAND_MAX_BYTES : (uint64_t)1 << 30;     // (dynamic: bit offsets fit 32 bits)
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, most / row));
}

unsigned char *PngEncoder::band_buffer(size_t bytes)
{
    HIP_TRY(hipSetDevice(device));
    grow(raster, raster_cap, bytes);
    return raster;
}

// ---- the host's part of a dynamic band: the code, its header, the piece's end ----------------------------------------
namespace {

// Optimal code lengths of at most `limit` bits for the symbols with counts above 0 (at least two of them): the Huffman tree
// where it is no deeper than that, else package-merge (Larmore & Hirschberg), which is optimal among the limited codes.
// Both are complete: the Kraft sum is exactly 1.
void code_lengths(const uint64_t *counts, uint32_t n, uint32_t limit, uint8_t *lens)
{
    std::vector<uint32_t> used;
    for (uint32_t i = 0; i < n; i++) { lens[i] = 0; if (counts[i]) used.push_back(i); }
    const uint32_t m = (uint32_t)used.size();
    if (m < 2) throw Error{MARAY_E_INTERNAL, "device PNG encoder: a code needs two symbols"};
    std::stable_sort(used.begin(), used.end(), [&](uint32_t x, uint32_t y) { return counts[x] < counts[y]; });
    // Huffman over the sorted leaves with two queues: node k < m is leaf k, the others are made in order of weight
    std::vector<uint64_t> wt(2 * m - 1);
    std::vector<uint32_t> parent(2 * m - 1, 0);
    for (uint32_t k = 0; k < m; k++) wt[k] = counts[used[k]];
    uint32_t leaf = 0, inner = m, made = m;
    auto take = [&]() { return leaf < m && (inner >= made || wt[leaf] <= wt[inner]) ? leaf++ : inner++; };
    while (made < 2 * m - 1) {
        const uint32_t x = take(), y = take();
        wt[made] = wt[x] + wt[y];
        parent[x] = parent[y] = made;
        made++;
    }
    std::vector<uint32_t> depth(2 * m - 1, 0);
    uint32_t deepest = 0;
    for (uint32_t k = 2 * m - 2; k-- > 0;) { depth[k] = depth[parent[k]] + 1; if (k < m) deepest = std::max(deepest, depth[k]); }
    if (deepest <= limit) {
        for (uint32_t k = 0; k < m; k++) lens[used[k]] = (uint8_t)depth[k];
        return;
    }
    // package-merge: an item is a weight and how often each leaf is in it; level by level the items are paired into packages
    // and merged with the leaves; the 2 m - 2 lightest items of the last level hold leaf k once per bit of its code
    struct Item { uint64_t w; std::vector<uint8_t> in; };
    std::vector<Item> leaves(m), prev;
    for (uint32_t k = 0; k < m; k++) { leaves[k].w = wt[k]; leaves[k].in.assign(m, 0); leaves[k].in[k] = 1; }
    prev = leaves;
    for (uint32_t level = 1; level < limit; level++) {
        std::vector<Item> packs;
        for (size_t i = 0; i + 1 < prev.size(); i += 2) {
            Item p{prev[i].w + prev[i + 1].w, prev[i].in};
            for (uint32_t k = 0; k < m; k++) p.in[k] = (uint8_t)(p.in[k] + prev[i + 1].in[k]);
            packs.push_back(std::move(p));
        }
        std::vector<Item> merged;
        size_t x = 0, y = 0;
        while (x < m || y < packs.size())
            merged.push_back(y >= packs.size() || (x < m && leaves[x].w <= packs[y].w) ? leaves[x++] : std::move(packs[y++]));
        prev = std::move(merged);
    }
    for (uint32_t i = 0; i < 2 * m - 2; i++)
        for (uint32_t k = 0; k < m; k++) lens[used[k]] = (uint8_t)(lens[used[k]] + prev[i].in[k]);
}

// canonical codes (RFC 1951, 3.2.2) of the lengths, as they stand in the code's own bit order
void canonical_codes(const uint8_t *lens, uint32_t n, uint32_t max_bits, uint32_t *codes)
{
    std::vector<uint32_t> count(max_bits + 2, 0), next(max_bits + 2, 0);
    for (uint32_t i = 0; i < n; i++) count[lens[i]]++;
    count[0] = 0;
    uint32_t code = 0;
    for (uint32_t b = 1; b <= max_bits; b++) { code = (code + count[b - 1]) << 1; next[b] = code; }
    for (uint32_t i = 0; i < n; i++) codes[i] = lens[i] ? next[lens[i]]++ : 0;
}

uint32_t reversed(uint32_t code, uint32_t bits)
{
    uint32_t r = 0;
    for (uint32_t b = 0; b < bits; b++) r |= ((code >> b) & 1u) << (bits - 1 - b);
    return r;
}

struct BitWriter {
    std::vector<uint8_t> &z;
    uint64_t bits;
    void put(uint32_t value, uint32_t n)                      // n <= 16 bits, LSB first
    {
        for (uint32_t b = 0; b < n; b++, bits++) {
            if ((bits >> 3) >= z.size()) z.push_back(0);
            z[(size_t)(bits >> 3)] = (uint8_t)(z[(size_t)(bits >> 3)] | (((value >> b) & 1u) << (bits & 7)));
        }
    }
};

// BFINAL = 0, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code, the lengths one by one (no run symbols); returns the bits
uint64_t dynamic_header(const uint8_t lit_lens[PNG_LIT_SYMS], const uint8_t dist_lens[PNG_DIST_SYMS], std::vector<uint8_t> &z)
{
    uint32_t n_lit = PNG_LIT_SYMS, n_dist = PNG_DIST_SYMS;
    while (n_lit > 257 && !lit_lens[n_lit - 1]) n_lit--;
    while (n_dist > 1 && !dist_lens[n_dist - 1]) n_dist--;
    uint64_t cl_counts[19] = {0};
    for (uint32_t i = 0; i < n_lit; i++) cl_counts[lit_lens[i]]++;
    for (uint32_t i = 0; i < n_dist; i++) cl_counts[dist_lens[i]]++;
    uint8_t cl_lens[19];
    uint32_t cl_codes[19];
    code_lengths(cl_counts, 19, 7, cl_lens);                  // (length 0 -- a distance symbol's at least -- and a used symbol's: two or more)
    canonical_codes(cl_lens, 19, 7, cl_codes);
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t n_cl = 19;
    while (n_cl > 4 && !cl_lens[order[n_cl - 1]]) n_cl--;
    z.clear();
    BitWriter bw{z, 0};
    bw.put(0, 1); bw.put(2, 2);
    bw.put(n_lit - 257, 5); bw.put(n_dist - 1, 5); bw.put(n_cl - 4, 4);
    for (uint32_t i = 0; i < n_cl; i++) bw.put(cl_lens[order[i]], 3);
    for (uint32_t i = 0; i < n_lit; i++) bw.put(reversed(cl_codes[lit_lens[i]], cl_lens[lit_lens[i]]), cl_lens[lit_lens[i]]);
    for (uint32_t i = 0; i < n_dist; i++) bw.put(reversed(cl_codes[dist_lens[i]], cl_lens[dist_lens[i]]), cl_lens[dist_lens[i]]);
    return bw.bits;
}

// the lengths of a band's two codes from its counts; throws MARAY_E_ARG for counts no band has
void dynamic_lengths(const uint32_t lit_counts[PNG_LIT_SYMS], const uint32_t dist_counts[PNG_DIST_SYMS], uint8_t lit_lens[PNG_LIT_SYMS],
                     uint8_t dist_lens[PNG_DIST_SYMS])
{
    uint64_t c[PNG_LIT_SYMS];
    uint32_t used = 0;
    for (uint32_t i = 0; i < PNG_LIT_SYMS; i++) { c[i] = lit_counts[i]; used += lit_counts[i] != 0; }
    if (!lit_counts[256] || used < 2) throw Error{MARAY_E_ARG, "dynamic codes: symbol 256 and at least one other symbol must occur"};
    for (uint32_t i = 0; i < PNG_DIST_SYMS; i++) {
        if (i != 2 && dist_counts[i]) throw Error{MARAY_E_ARG, "dynamic codes: every match is at distance 3 (distance symbol 2)"};
        dist_lens[i] = 0;
    }
    code_lengths(c, PNG_LIT_SYMS, 15, lit_lens);
    if (dist_counts[2]) dist_lens[2] = 1;
}

}   // namespace

void png_dynamic_table(const uint8_t lit_lens[PNG_LIT_SYMS], uint32_t table[PNG_LIT_SYMS])
{
    uint32_t codes[PNG_LIT_SYMS];
    canonical_codes(lit_lens, PNG_LIT_SYMS, 15, codes);
    for (uint32_t i = 0; i < PNG_LIT_SYMS; i++) table[i] = reversed(codes[i], lit_lens[i]) | ((uint32_t)lit_lens[i] << 16);
}

void png_dynamic_close(std::vector<uint8_t> &z, uint64_t bits, uint32_t code256, size_t base)
{
    bits += 8 * (uint64_t)base;
    z.resize((size_t)((bits + 7) / 8));
    BitWriter bw{z, bits};
    bw.put(code256 & 0xFFFFu, code256 >> 16);
    bw.put(0, 3);                                             // BFINAL = 0, BTYPE = 00; the rest of the byte is zero already
    z.resize((size_t)((bw.bits + 7) / 8));
    static const uint8_t sync[4] = {0x00, 0x00, 0xFF, 0xFF};
    z.insert(z.end(), sync, sync + 4);
}

extern "C" int maray_png_dynamic_codes(const uint32_t lit_counts[286], const uint32_t dist_counts[30], uint8_t lit_lens[286], uint8_t dist_lens[30],
                                       uint8_t *header, size_t cap, size_t *header_bits)
{
    try {
        if (!lit_counts || !dist_counts || !lit_lens || !dist_lens || !header || !header_bits) throw Error{MARAY_E_ARG, "null argument"};
        *header_bits = 0;
        dynamic_lengths(lit_counts, dist_counts, lit_lens, dist_lens);
        std::vector<uint8_t> z;
        const uint64_t bits = dynamic_header(lit_lens, dist_lens, z);
        if (z.size() > cap) throw Error{MARAY_E_ARG, "dynamic codes: the header does not fit the buffer"};
        memcpy(header, z.data(), z.size());
        *header_bits = (size_t)bits;
        set_last_error("");
        return MARAY_OK;
    }
    catch (const Error &e) { set_last_error(e.msg); return e.code; }
    catch (const std::exception &e) { set_last_error(e.what()); return MARAY_E_INTERNAL; }
}

void PngEncoder::encode_rows(const unsigned char *d_rgb8, uint32_t w, uint32_t rows, hipStream_t st, PngPiece &out, uint32_t codes, uint32_t filter,
                             const unsigned char *above)
{
    if (codes != MARAY_PNG_CODES_FIXED && codes != MARAY_PNG_CODES_DYNAMIC) throw Error{MARAY_E_ARG, "unknown PNG codes"};
    if (!png_filter_known(filter)) throw Error{MARAY_E_ARG, "unknown PNG filter"};
    if (!rows || !w) return;
    if (!d_rgb8) throw Error{MARAY_E_ARG, "null argument"};
    HIP_TRY(hipSetDevice(device));
    const bool dyn = codes == MARAY_PNG_CODES_DYNAMIC;
    const uint32_t step = band_rows(w, codes);
    std::vector<uint8_t> header;
    for (uint32_t r0 = 0; r0 < rows; r0 += std::min(step, rows - r0)) {
        const uint32_t n = std::min(step, rows - r0);
        // (a band after the first has the row above it in the raster: src - 3 w)
        PngBandArgs a = band_args(*this, d_rgb8 + (size_t)r0 * w * 3, w, n, codes, filter, r0 ? d_rgb8 + (size_t)(r0 - 1) * w * 3 : above);
        uint32_t code256 = 0;
        if (dyn) {
            // count the band's tokens, fit the code on the host, hand the device its table and the header's length
            const uint32_t blocks = png_hist_blocks(a.n_segs);
            uint32_t *d_sums = a.hist + (size_t)blocks * PNG_HIST_STRIDE, *d_table = d_sums + PNG_HIST_STRIDE;
            png_band_compress(a, st);
            HIP_TRY(hipMemcpyAsync(h_counts, d_sums, PNG_HIST_STRIDE * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            uint32_t dist_counts[PNG_DIST_SYMS] = {0};
            for (uint32_t s = 257; s < PNG_LIT_SYMS; s++) dist_counts[2] += h_counts[s];       // every match is at distance 3
            h_counts[256] = 1;
            uint8_t lit_lens[PNG_LIT_SYMS], dist_lens[PNG_DIST_SYMS];
            dynamic_lengths(h_counts, dist_counts, lit_lens, dist_lens);
            a.header_bits = (uint32_t)dynamic_header(lit_lens, dist_lens, header);
            uint32_t *h_table = h_counts + PNG_HIST_STRIDE;
            png_dynamic_table(lit_lens, h_table);
            code256 = h_table[256];
            HIP_TRY(hipMemcpyAsync(d_table, h_table, PNG_LIT_SYMS * 4, hipMemcpyHostToDevice, st));
            a.table = d_table;
            g_bytes_to_host += PNG_HIST_STRIDE * 4;
        }
        png_band_compress(a, st);
        png_band_scan(a, st);
        png_band_gather(a, st);
        HIP_TRY(hipMemcpyAsync(h_totals, a.totals, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        // fixed: the band's bytes; dynamic: its tokens' bits, behind the header's
        const uint64_t total = dyn ? (a.header_bits + h_totals[0] + 7) / 8 : h_totals[0];
        if ((dyn ? h_totals[0] / 8 : total) > (uint64_t)a.n_segs * a.slot_bytes) throw Error{MARAY_E_INTERNAL, "device PNG encoder: a band's stream exceeds its bound"};
        want_staging((size_t)total);
        HIP_TRY(hipMemcpyAsync(staging, a.stream, (size_t)total, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const size_t base = out.z.size();
        out.z.insert(out.z.end(), staging, staging + (size_t)total);
        if (dyn) {
            for (size_t i = 0; i < header.size(); i++) out.z[base + i] |= header[i];      // (the device left the header's bits zero)
            png_dynamic_close(out.z, a.header_bits + h_totals[0], code256, base);
        }
        AdlerPart p;
        p.n = (uint32_t)(h_totals[1] & 0xFFFFFFFFu); p.a = (uint32_t)(h_totals[1] >> 32); p.b = (uint32_t)h_totals[2];
        out.adler.append(p);
        g_bytes_to_host += total + 24;
    }
}

void PngEncoder::want_staging(size_t bytes)
{
    if (bytes <= staging_cap) return;
    if (staging) HIP_TRY(hipHostFree(staging));
    staging = nullptr; staging_cap = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 4, (size_t)1 << 20);
    HIP_TRY(hipHostMalloc((void **)&staging, want, hipHostMallocDefault));
    staging_cap = want;
}

void PngEncoder::encode_rendered(uint32_t w, uint32_t y0, uint32_t y1, hipStream_t st,
                                 const std::function<void(uint32_t, uint32_t, unsigned char *, hipStream_t)> &render, PngPiece &out, uint32_t codes,
                                 uint32_t filter)
{
    if (codes != MARAY_PNG_CODES_FIXED && codes != MARAY_PNG_CODES_DYNAMIC) throw Error{MARAY_E_ARG, "unknown PNG codes"};
    if (!png_filter_known(filter)) throw Error{MARAY_E_ARG, "unknown PNG filter"};
    if (y0 >= y1 || !w) return;
    HIP_TRY(hipSetDevice(device));
    const uint32_t step = band_rows(w, codes);
    grow(raster, raster_cap, (size_t)std::min(step, y1 - y0) * w * 3);
    const bool filtered = filter != MARAY_PNG_FILTER_NONE;
    const size_t row_bytes = (size_t)w * 3;
    const unsigned char *above = nullptr;
    // (a filtered piece starts the image: the row above y0 > 0 would have to be rendered first, and no caller needs it)
    if (filtered && y0 > 0) throw Error{MARAY_E_INTERNAL, "device PNG encoder: a filtered piece must start at row 0"};
    if (filtered) grow(carry, carry_cap, row_bytes);
    for (uint32_t b0 = y0; b0 < y1; b0 += std::min(step, y1 - b0)) {
        const uint32_t b1 = b0 + std::min(step, y1 - b0);
        render(b0, b1, raster, st);
        HIP_TRY(hipSetDevice(device));
        encode_rows(raster, w, b1 - b0, st, out, codes, filter, above);
        if (filtered && b1 < y1) {
            // the band's last row, before the next band's render overwrites the band buffer (the same stream: in order)
            HIP_TRY(hipMemcpyAsync(carry, raster + (size_t)(b1 - b0 - 1) * row_bytes, row_bytes, hipMemcpyDeviceToDevice, st));
            above = carry;
        }
    }
}

// ---- the encoders a process keeps ------------------------------------------------------------------------------------
namespace {
std::mutex g_pool_mutex;
// never destroyed: at process exit the HIP runtime may be gone before a static's destructor runs
std::multimap<int, PngEncoder *> &g_pool = *new std::multimap<int, PngEncoder *>();
}   // namespace

PngEncoder *png_encoder_acquire(int device)
{
    const uint32_t env = band_rows_from_env();
    std::vector<PngEncoder *> stale;
    PngEncoder *e = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        for (auto it = g_pool.lower_bound(device); it != g_pool.end() && it->first == device && !e;) {
            if (it->second->band_rows_env == env) e = it->second; else stale.push_back(it->second);
            it = g_pool.erase(it);
        }
    }
    for (PngEncoder *s : stale) delete s;
    return e ? e : new PngEncoder(device);
}

void png_encoder_release(PngEncoder *e)
{
    if (!e) return;
    {
        std::lock_guard<std::mutex> lk(g_pool_mutex);
        if (g_pool.count(e->device) < 2) { g_pool.insert({e->device, e}); return; }
    }
    delete e;
}

uint64_t png_bytes_to_host() { return g_bytes_to_host.load(); }
void png_count_bytes_to_host(uint64_t n) { g_bytes_to_host += n; }

void png_check_size(uint32_t w, uint32_t h)
{
    if (w > MARAY_DOMAIN_MAX || h > MARAY_DOMAIN_MAX || ((uint64_t)w * 3 + 1) * h > MARAY_PNG_MAX_BYTES)
        throw Error{MARAY_E_LIMIT, "image too large for the PNG writer"};
}

std::vector<uint8_t> png_close_stream(uint32_t h_end, const std::vector<const PngPiece *> &pieces)
{
    size_t zn = 2 + 5 + 4;
    uint32_t y = pieces.empty() ? 0 : pieces.front()->y0;
    for (const PngPiece *p : pieces) {
        if (p->y0 != y || p->y1 <= p->y0) throw Error{MARAY_E_INTERNAL, "device PNG encoder: the pieces do not cover the image in row order"};
        y = p->y1;
        zn += p->z.size();
    }
    if (pieces.empty() || y != h_end) throw Error{MARAY_E_INTERNAL, "device PNG encoder: the pieces do not cover the image"};
    std::vector<uint8_t> z;
    z.reserve(zn);
    z.push_back(0x78); z.push_back(0x01);
    uint32_t s1 = 1, s2 = 0;
    for (const PngPiece *p : pieces) {
        z.insert(z.end(), p->z.begin(), p->z.end());
        s2 = (uint32_t)(((uint64_t)s2 + (uint64_t)p->adler.n * s1 + p->adler.b) % PNG_ADLER_MOD);
        s1 = (s1 + p->adler.a) % PNG_ADLER_MOD;
    }
    static const uint8_t last[5] = {0x01, 0x00, 0x00, 0xFF, 0xFF};       // the final, empty stored block
    z.insert(z.end(), last, last + 5);
    put_be32(z, (s2 << 16) | s1);
    return z;
}

std::vector<uint8_t> png_assemble(uint32_t w, uint32_t h, const std::vector<const PngPiece *> &pieces)
{
    if (!pieces.empty() && pieces.front()->y0 != 0) throw Error{MARAY_E_INTERNAL, "device PNG encoder: the pieces do not cover the image in row order"};
    const std::vector<uint8_t> z = png_close_stream(h, pieces);
    return png_file(w, h, z.data(), z.size());
}

float png_time_kernels(int device, const unsigned char *d_rgb8, uint32_t w, uint32_t rows, int reps, uint64_t *stream_bytes, uint32_t codes,
                       uint32_t filter)
{
    if (codes != MARAY_PNG_CODES_FIXED && codes != MARAY_PNG_CODES_DYNAMIC) throw Error{MARAY_E_ARG, "unknown PNG codes"};
    if (!png_filter_known(filter)) throw Error{MARAY_E_ARG, "unknown PNG filter"};
    const bool dyn = codes == MARAY_PNG_CODES_DYNAMIC;
    if (!d_rgb8 || !w || !rows || reps <= 0) throw Error{MARAY_E_ARG, "png_time_kernels: a raster, w, rows and reps > 0"};
    png_check_size(w, rows);
    if (((uint64_t)w * 3 + 1) * rows > (dyn ? PNG_DYN_BAND_MAX_BYTES : (uint64_t)1 << 30)) throw Error{MARAY_E_LIMIT, "png_time_kernels: more than one band's bytes"};
    PngEncoderLease E(device);
    HIP_TRY(hipSetDevice(device));
    PngBandArgs a = band_args(*E.e, d_rgb8, w, rows, codes, filter);
    const hipStream_t st = E->own_stream;
    PngBandArgs count = a;                      // dynamic: the counting pass; `a` gets the code fitted to its counts once
    uint32_t len256 = 0;
    if (dyn) {
        const uint32_t blocks = png_hist_blocks(a.n_segs);
        uint32_t *d_sums = a.hist + (size_t)blocks * PNG_HIST_STRIDE, *d_table = d_sums + PNG_HIST_STRIDE;
        png_band_compress(count, st);
        HIP_TRY(hipMemcpyAsync(E->h_counts, d_sums, PNG_HIST_STRIDE * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        uint32_t dist_counts[PNG_DIST_SYMS] = {0};
        for (uint32_t s = 257; s < PNG_LIT_SYMS; s++) dist_counts[2] += E->h_counts[s];
        E->h_counts[256] = 1;
        uint8_t lit_lens[PNG_LIT_SYMS], dist_lens[PNG_DIST_SYMS];
        dynamic_lengths(E->h_counts, dist_counts, lit_lens, dist_lens);
        std::vector<uint8_t> header;
        a.header_bits = (uint32_t)dynamic_header(lit_lens, dist_lens, header);
        png_dynamic_table(lit_lens, E->h_counts + PNG_HIST_STRIDE);
        len256 = lit_lens[256];
        HIP_TRY(hipMemcpyAsync(d_table, E->h_counts + PNG_HIST_STRIDE, PNG_LIT_SYMS * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        a.table = d_table;
    }
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    HIP_TRY(hipEventCreate(&ev.e0)); HIP_TRY(hipEventCreate(&ev.e1));
    auto once = [&] { if (dyn) png_band_compress(count, st); png_band_compress(a, st); png_band_scan(a, st); png_band_gather(a, st); };
    once();
    HIP_TRY(hipEventRecord(ev.e0, st));
    for (int i = 0; i < reps; i++) once();
    HIP_TRY(hipEventRecord(ev.e1, st));
    HIP_TRY(hipMemcpyAsync(E->h_totals, a.totals, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (dynamic: the header, the tokens, symbol 256 and the sync's three bits, zeros to the byte, four bytes)
    if (stream_bytes) *stream_bytes = dyn ? (a.header_bits + E->h_totals[0] + len256 + 3 + 7) / 8 + 4 : E->h_totals[0];
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    return ms / (float)reps;
}

}   // namespace maray
